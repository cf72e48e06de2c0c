"""Graph-replayed decoding on the GPU: ``generate(useGraph=True)`` (the step captured once into a HIP graph and
replayed), its eager twin ``pinPositions=True`` and the ordinary call give the same bits while the decode attention
runs one split; across the split boundary graph == pinned eager bitwise and pinned == ordinary within the decode
kernel's bound. The commit kernel of csrc/generation.hip alone against its torch twin."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer, TransformerSeq2Seq
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import generation_native as GN
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
V, HEADS, HS = 97, 2, 64
CACHED = ("decoder_0", "decoder_1")


@functools.lru_cache(maxsize=None)
def _lm():
    return TextGenerationTransformer(numLabels=V, hidden=HEADS * HS, layers=2, heads=HEADS, inputShape=[16],
                                     maxPositions=512, seed=5, dataType=DataType.BFLOAT16).init(device=DEV)


@functools.lru_cache(maxsize=None)
def _s2s():
    return TransformerSeq2Seq(numLabels=V, hidden=HEADS * HS, layers=2, heads=HEADS, inputShape=[8, 16],
                              maxPositions=512, seed=6, dataType=DataType.BFLOAT16).init(device=DEV)


def _prompt(mb, Tp, seed=0):
    return torch.randint(0, V, (mb, Tp), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _same(a, b):
    return torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.scores, b.scores)


def _one_split(mb, Tp, N):
    """The precondition of the bitwise comparisons against the ordinary call: one split under the host's own bound
    at every step and under the pinned bound (then the ragged kernel is the uniform kernel at the row's position)."""
    assert Tp + N <= 128
    for L in range(1, Tp + N + 1):
        assert TN.attn_decode_splits(mb, 1, HEADS, HS, L) == 1


def _err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


# ------------------------------------------------------------------------------------------------ 1: greedy
def test_greedy_graph_equals_pinned_equals_ordinary_and_the_appends_land_in_the_right_rows():
    net, mb, Tp, N = _lm(), 3, 5, 24
    _one_split(mb, Tp, N)
    prompt = _prompt(mb, Tp)
    want = net.generate(prompt, maxNewTokens=N)
    kv_want = {n: net.rnnGetPreviousState(n)["kv"] for n in CACHED}
    pinned = net.generate(prompt, maxNewTokens=N, pinPositions=True)
    assert net.lastGenerationStats == {"captures": 0, "graphReplays": 0, "eagerSteps": N}
    got = net.generate(prompt, maxNewTokens=N, useGraph=True)
    st = net.lastGenerationStats
    print("stats", st)
    assert _same(pinned, want) and _same(got, want)
    assert st["captures"] == 1 and st["graphReplays"] > 0 and st["graphReplays"] + st["eagerSteps"] == N
    real = Tp + N - 1                                            # every row fed its prompt and N - 1 tokens
    for n in CACHED:
        state = net.rnnGetPreviousState(n)
        assert kv_want[n].shape[1] == real
        assert torch.equal(state["kv"][:, :real], kv_want[n]), f"{n}: the cache differs from the ordinary call's"
        assert torch.equal(state["short"].cpu(), torch.full((mb,), state["kv"].shape[1] - real, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ 2: sampling, eos
def test_seeded_sampling_with_eos_and_padding():
    net, mb, Tp, N = _lm(), 3, 5, 24
    _one_split(mb, Tp, N)
    prompt = _prompt(mb, Tp, 1)
    kw = dict(maxNewTokens=N, doSample=True, temperature=0.8, topK=20, topP=0.9, seed=11, eosCheckEvery=4)
    eos = int(net.generate(prompt, **kw).tokens[0, 5])
    kw.update(eosToken=eos, padToken=V - 1)
    want = net.generate(prompt, **kw)
    assert int(want.lengths[0]) <= 6 and (want.tokens[0, int(want.lengths[0]):] == V - 1).all()
    got = net.generate(prompt, useGraph=True, **kw)
    assert net.lastGenerationStats["captures"] == 1
    again = net.generate(prompt, useGraph=True, **kw)
    assert _same(got, want) and _same(again, got)
    assert _same(net.generate(prompt, pinPositions=True, **kw), want)


# ------------------------------------------------------------------------------------------------ 3: ragged
@pytest.mark.parametrize("kw", [dict(), dict(doSample=True, temperature=0.8, topK=20, topP=0.9, seed=7)],
                         ids=["greedy", "sampling"])
def test_ragged_prompts(kw):
    net, Tp, lens, N = _lm(), 65, (1, 5, 64, 65), 20
    _one_split(len(lens), Tp, N)
    prompt = _prompt(len(lens), Tp, 2)
    want = net.generate(prompt, promptLengths=lens, maxNewTokens=N, **kw)
    pinned = net.generate(prompt, promptLengths=lens, maxNewTokens=N, pinPositions=True, **kw)
    got = net.generate(prompt, promptLengths=lens, maxNewTokens=N, useGraph=True, **kw)
    assert net.lastGenerationStats["captures"] == 1
    assert _same(pinned, want) and _same(got, want)


# ------------------------------------------------------------------------------------------------ 4: seq2seq
def test_seq2seq_with_a_source_mask():
    net, mb, N = _s2s(), 3, 20
    _one_split(mb, 1, N)
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, V, (mb, 6), generator=g).to(DEV)
    smask = torch.tensor([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0]], dtype=torch.float32).to(DEV)
    start = torch.randint(0, V, (mb, 1), generator=g).to(DEV)
    want = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=N)
    got = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=N, useGraph=True)
    assert net.lastGenerationStats["captures"] == 1 and net.lastGenerationStats["graphReplays"] > 0
    assert _same(got, want)


# ------------------------------------------------------------------------------------------------ 5: split boundary
def _step(net, x):
    return net.rnnTimeStep(x)[0]


def test_across_the_split_boundary():
    """Tp 120 + 80 new tokens: 4 key blocks under the pinned bound, so the pinned steps may run more splits than the
    ordinary ones and owe them the decode kernel's bound (tests/test_gpu_attention_decode.py), not their bits."""
    net, mb, Tp, N = _lm(), 3, 120, 80
    prompt = _prompt(mb, Tp, 4)
    pinned = net.generate(prompt, maxNewTokens=N, pinPositions=True)
    got = net.generate(prompt, maxNewTokens=N, useGraph=True)
    assert net.lastGenerationStats["captures"] == 1
    assert _same(got, pinned)
    toks = net.generate(prompt, maxNewTokens=N).tokens
    net.rnnClearPreviousState()
    _step(net, prompt)
    want = [_step(net, toks[:, t:t + 1]) for t in range(N - 1)]
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnPinState(Tp + N)
    worst = 0.0
    for t in range(N - 1):
        worst = max(worst, _err(_step(net, toks[:, t:t + 1]), want[t]))
    print(f"pinned vs ordinary distributions over {N - 1} steps: worst err {worst:.3e}")
    assert worst < 2e-2
    net.rnnClearPreviousState()


# ------------------------------------------------------------------------------------------------ 6: hygiene
def test_state_hygiene_after_a_graph_call():
    net = _lm()
    fallback.reset()
    net.generate(_prompt(3, 5), maxNewTokens=12, useGraph=True)
    assert net.lastGenerationStats["captures"] == 1
    assert net.helperCountFail() == 0, net.fallbackSummary()
    fresh = TextGenerationTransformer(numLabels=V, hidden=HEADS * HS, layers=2, heads=HEADS, inputShape=[16],
                                      maxPositions=512, seed=5, dataType=DataType.BFLOAT16).init(device=DEV)
    with torch.no_grad():
        fresh.flattenedParams.copy_(net.flattenedParams)
    prompt = _prompt(2, 7, 9)
    assert _same(net.generate(prompt, maxNewTokens=9), fresh.generate(prompt, maxNewTokens=9))


# ------------------------------------------------------------------------------------------------ 7: commit kernel
@pytest.mark.parametrize("record", [False, True], ids=["advance", "advance+record"])
@pytest.mark.parametrize("mb", [1, 3, 257])
def test_commit_kernel_against_its_torch_twin(mb, record):
    g = torch.Generator().manual_seed(mb)
    short0 = torch.randint(0, 7, (mb,), generator=g, dtype=torch.int32)
    short0[:3] = torch.tensor([5, 0, 2], dtype=torch.int32)[:mb]
    N = 2                                                        # the third launch finds the buffers full

    def run(dev, commit):
        short = short0.clone().to(dev)
        rec = None
        if record:
            rec = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(mb, dtype=torch.int64, device=dev),
                   torch.zeros(mb, dtype=torch.float32, device=dev),
                   torch.full((N, mb), -1, dtype=torch.int64, device=dev),
                   torch.full((N, mb), -1.0, dtype=torch.float32, device=dev))
        seen = []
        for i in range(3):
            if record:
                rec[1].copy_(torch.arange(mb) + 100 * (i + 1))
                rec[2].copy_(-(torch.arange(mb, dtype=torch.float32) + 0.5 * i))
            commit(short, rec)
            seen.append([short.cpu().clone()] + ([t.cpu().clone() for t in (rec[0], rec[3], rec[4])] if record else []))
        return seen

    fallback.reset()
    got = run(DEV, GN.step_commit)
    assert fallback.count() == 0, fallback.summary()
    want = run(torch.device("cpu"), GN.step_commit_torch)
    for i, (a, b) in enumerate(zip(got, want)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), f"launch {i}"
        assert torch.equal(a[0], (short0 - (i + 1)).clamp(min=0))                    # floors at 0
        if record:
            assert int(a[1]) == min(i + 1, N)
            assert (a[2][:min(i + 1, N)] >= 100).all() and (a[2][min(i + 1, N):] == -1).all()
    if record:
        assert torch.equal(got[2][2], got[1][2]) and torch.equal(got[2][3], got[1][3])  # nothing written at t == N
        step = torch.zeros(1, dtype=torch.int32, device=DEV)                         # the record part alone
        toks = torch.full((N, mb), -1, dtype=torch.int64, device=DEV)
        lps = torch.zeros(N, mb, dtype=torch.float32, device=DEV)
        GN.step_commit(None, (step, torch.arange(mb, device=DEV), torch.ones(mb, device=DEV), toks, lps))
        assert int(step) == 1 and torch.equal(toks[0].cpu(), torch.arange(mb)) and (toks[1] == -1).all()
        assert fallback.count() == 0, fallback.summary()
