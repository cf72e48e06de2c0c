"""Speculative decoding on the CPU (fp64 networks, where chunked and single-step arithmetic agree far below any argmax
margin): generate(numDraftTokens=K) with an assistant and with prompt lookup against plain generate(), the torch twins
of csrc/speculative.hip (verify, commit, n-gram draft) and rnnSetPositions."""
import math

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.models import TextGenerationLSTM, TransformerSeq2Seq
from deeplearning4j_amd.ops import generation_native as GN

CPU = torch.device("cpu")
V, K, N = 23, 3, 14


def _lm(layers=2, seed=5, vocab=V, heads=2, maxPositions=64):
    """A MultiLayerNetwork language model: position embeddings, ``layers`` causal blocks of 2 x 64 (1 x 128), softmax."""
    b = (NeuralNetConfiguration.Builder().seed(seed).dataType(DataType.DOUBLE).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.3)).list())
    b.layer(0, BertEmbeddingLayer.Builder().nIn(vocab).nOut(128).maxPositions(maxPositions).inputLength(8).build())
    for i in range(layers):
        b.layer(1 + i, TransformerEncoderLayer.Builder().nIn(128).nOut(128).nHeads(heads).ffnSize(64).causal(True)
                .build())
    b.layer(1 + layers, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(128)
            .nOut(vocab).build())
    net = MultiLayerNetwork(b.build())
    net.init(device=CPU)
    return net


def _s2s(layers=2, seed=6):
    return TransformerSeq2Seq(numLabels=V, hidden=128, layers=layers, heads=2, inputShape=[8, 16], maxPositions=64,
                              seed=seed, dataType=DataType.DOUBLE).init(device=CPU)


@pytest.fixture(scope="module")
def lms():
    """target, a different random 1-block assistant, a copy of the target, a 1 x 128 target."""
    return {"net": _lm(), "other": _lm(layers=1, seed=9), "copy": _lm(), "wide": _lm(heads=1)}


PROMPT = torch.randint(0, V, (3, 6), generator=torch.Generator().manual_seed(1))
LENGTHS = torch.tensor([6, 3, 4])


def _mid_eos(tokens):
    """A token that stops some row in the middle of its sequence and no row at once: among the tokens emitted, the
    one whose earliest first occurrence over the rows is the latest."""
    n = tokens.shape[1]
    first = {int(t): min(int((row == t).int().argmax()) if bool((row == t).any()) else n for row in tokens)
             for t in tokens.unique()}
    return max(first, key=lambda t: (first[t] if first[t] < n - 1 else -1, -t))


def _same(r, want):
    assert torch.equal(r.tokens, want.tokens) and torch.equal(r.lengths, want.lengths)
    assert float((r.scores.double() - want.scores.double()).abs().max()) <= 1e-9


# ------------------------------------------------------------------------------------------------ generate()
@pytest.mark.parametrize("source", ["other", "copy", "lookup"])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("eos", [False, True])
def test_greedy_speculative_equals_plain_generate(lms, source, ragged, eos):
    net = lms["net"]
    kw = dict(promptLengths=LENGTHS) if ragged else {}
    free = net.generate(PROMPT, maxNewTokens=N, **kw)
    if eos:
        kw.update(eosToken=_mid_eos(free.tokens), padToken=V - 1)
    want = net.generate(PROMPT, maxNewTokens=N, **kw)
    if eos:
        assert 2 < int(want.lengths.min()) < N
    r = net.generate(PROMPT, maxNewTokens=N, numDraftTokens=K, assistant=lms.get(source), **kw)
    _same(r, want)
    st = net.lastGenerationStats
    assert set(st) == {"rounds", "draftTokens", "acceptedTokens"} and 0 <= st["acceptedTokens"] <= st["draftTokens"]
    if source == "other" and not eos:
        assert st["acceptedTokens"] < st["draftTokens"], "the assistant never disagreed: rejections not exercised"


def test_greedy_speculative_on_the_one_head_model_and_other_draft_sizes(lms):
    net = lms["wide"]
    want = net.generate(PROMPT, maxNewTokens=N, promptLengths=LENGTHS)
    for k, ngram in ((1, 1), (2, 3), (4, 8)):
        _same(net.generate(PROMPT, maxNewTokens=N, promptLengths=LENGTHS, numDraftTokens=k, draftNgram=ngram), want)
        _same(net.generate(PROMPT, maxNewTokens=N, promptLengths=LENGTHS, numDraftTokens=k, assistant=lms["other"]),
              want)
    _same(net.generate(PROMPT, maxNewTokens=1, numDraftTokens=2), net.generate(PROMPT, maxNewTokens=1))


@pytest.mark.parametrize("source", ["other", "copy", "lookup"])
def test_greedy_speculative_seq2seq(source):
    net = _s2s()
    assistant = {"other": _s2s(layers=1, seed=8), "copy": _s2s(), "lookup": None}[source]
    g = torch.Generator().manual_seed(4)
    src = torch.randint(0, V, (2, 6), generator=g)
    smask = torch.tensor([[1., 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    start = torch.randint(0, V, (2, 3), generator=g)
    for kw in ({}, dict(startLengths=torch.tensor([3, 1]))):
        free = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=10, **kw)
        for eos in (None, _mid_eos(free.tokens)):
            want = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=10, eosToken=eos, **kw)
            r = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=10, eosToken=eos,
                                            numDraftTokens=K, assistant=assistant, **kw)
            _same(r, want)


@pytest.mark.parametrize("sample", [False, True])
def test_a_copy_of_the_target_has_every_draft_accepted(lms, sample):
    net = lms["net"]
    kw = dict(doSample=True, temperature=0.8, seed=11) if sample else {}
    for n, k in ((N, K), (13, 3), (9, 1), (24, 4)):
        net.generate(PROMPT, maxNewTokens=n, numDraftTokens=k, assistant=lms["copy"], **kw)
        st = net.lastGenerationStats
        assert st["rounds"] == math.ceil((n - 1) / (k + 1)), (n, k, st)
        assert st["acceptedTokens"] == st["draftTokens"] > 0, (n, k, st)


@pytest.mark.parametrize("source", ["other", "lookup"])
def test_seeded_sampling_gives_the_same_bits_twice(lms, source):
    net = lms["net"]
    kw = dict(maxNewTokens=N, numDraftTokens=K, assistant=lms.get(source), doSample=True, temperature=0.8,
              promptLengths=LENGTHS)
    a, b, c = (net.generate(PROMPT, seed=s, **kw) for s in (3, 3, 4))
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.scores, b.scores) and torch.equal(a.lengths, b.lengths)
    assert not torch.equal(a.tokens, c.tokens)
    assert bool(((a.tokens >= 0) & (a.tokens < V)).all()) and bool(torch.isfinite(a.scores).all())


# ------------------------------------------------------------------------------------------------ verify twin
def _verify(p, q, d, u, greedy=False, temperature=1.0, eos=None, pad=0, n=8, cursor=0, length=5, finished=None,
            hist=False):
    """Run the verify twin on fresh state -> dict of everything it updates. p [mb, K+1, V], q [mb, K, V] or None."""
    mb = p.shape[0]
    st = {"len": torch.full((mb,), length, dtype=torch.int32), "cursor": torch.full((mb,), cursor, dtype=torch.int32),
          "fin": torch.zeros(mb, dtype=torch.uint8) if finished is None else torch.tensor(finished, dtype=torch.uint8),
          "tokens": torch.full((mb, n), -1, dtype=torch.int64), "logps": torch.zeros(mb, n),
          "next": torch.full((mb,), -1, dtype=torch.int64), "counters": torch.zeros(2, dtype=torch.int32),
          "hist": torch.full((mb, length + n + 1), -1, dtype=torch.int64) if hist else None}
    GN.spec_verify_torch(p, q, d, u, temperature, greedy, st["len"], st["cursor"], st["fin"], eos, pad, st["tokens"],
                         st["logps"], st["next"], None, st["hist"], st["counters"])
    return st


def _tempered(x, temperature):
    w = x.double() ** (1.0 / temperature)
    return w / w.sum(-1, keepdim=True)


@pytest.mark.parametrize("given", ["random q", "q = null"])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_verify_twin_emits_the_targets_distribution(given, temperature):
    """Leviathan et al.: whatever the draft distribution, the first emitted token follows p~. R rows share p and q,
    the draft of every row is drawn from q~ (or is one fixed token for q = null, which is then one-hot there)."""
    R, Vs = 65536, 8
    g = torch.Generator().manual_seed(7)
    p = torch.softmax(1.5 * torch.randn(2, Vs, generator=g), 1)
    q = torch.softmax(1.5 * torch.randn(1, Vs, generator=g), 1)
    pt = _tempered(p[0], temperature)
    if given == "q = null":
        d = torch.full((R, 1), 2, dtype=torch.int64)
        qq = None
    else:
        d = torch.multinomial(_tempered(q[0], temperature), R, replacement=True, generator=g).reshape(R, 1)
        qq = q.reshape(1, 1, Vs).expand(R, 1, Vs)
    u = torch.rand(R, 4, generator=g)
    st = _verify(p.reshape(1, 2, Vs).expand(R, 2, Vs), qq, d, u, temperature=temperature)
    first = st["tokens"][:, 0]
    freq = torch.bincount(first, minlength=Vs).double() / R
    for v in range(Vs):
        bound = 5 * math.sqrt(float(pt[v]) * (1 - float(pt[v])) / R)
        print(f"{given} T={temperature} v={v}: freq {float(freq[v]):.5f} p~ {float(pt[v]):.5f} bound {bound:.5f}")
        assert abs(float(freq[v]) - float(pt[v])) <= bound
    # an accepted draft is followed by the bonus token: cursor 2, else 1
    acc = first == d[:, 0]
    assert torch.equal(st["cursor"], torch.where(st["tokens"][:, 1] >= 0, 2, 1).int()) and bool(acc.any())


def test_verify_twin_exact_cases():
    g = torch.Generator().manual_seed(3)
    Vs, Kk = 8, 3
    p = torch.softmax(torch.randn(2, Kk + 1, Vs, generator=g), 2)
    d = torch.tensor([[1, 2, 3], [4, 5, 6]])
    u = torch.rand(2, 2 * Kk + 2, generator=g)
    # q == p accepts all (u < 1): K + 1 tokens, the drafts first
    st = _verify(p, p[:, :Kk], d, u, hist=True)
    assert st["cursor"].tolist() == [4, 4] and st["len"].tolist() == [9, 9] and st["fin"].tolist() == [0, 0]
    assert torch.equal(st["tokens"][:, :3], d) and st["counters"].tolist() == [6, 6]
    assert torch.equal(st["next"], st["tokens"][:, 3]) and torch.equal(st["hist"][:, 6:10], st["tokens"][:, :4])
    want = torch.log(p.float().gather(2, st["tokens"][:, :4].reshape(2, 4, 1)))[:, :, 0]
    assert torch.equal(st["logps"][:, :4], want)
    # p_i(d_i) = 0 rejects at i, whatever u: here i = 1 in row 0
    p0 = p.clone()
    p0[0, 1, 2] = 0.0
    st = _verify(p0, p[:, :Kk], d, torch.zeros_like(u))
    assert st["cursor"].tolist() == [2, 4] and int(st["tokens"][0, 0]) == 1 and int(st["tokens"][0, 1]) != 2
    assert st["counters"].tolist() == [6, 4] and st["len"].tolist() == [7, 9]
    # a residual with one nonzero entry emits that entry: p and q differ only by moving mass from token 6 to token 0
    q1 = p[:, :Kk].clone()
    q1[:, 0, 0] += q1[:, 0, 6] - 0.001
    q1[:, 0, 6] = 0.001
    st = _verify(p, q1, torch.tensor([[0, 2, 3], [0, 5, 6]]), torch.full_like(u, 0.999))
    assert st["tokens"][:, 0].tolist() == [6, 6] and st["cursor"].tolist() == [1, 1]
    # a zero residual (q == p, but the draft token is outside the vocabulary: rejected) draws from p~
    ud = torch.rand(2, 2 * Kk + 2, generator=g)
    st = _verify(p, p[:, :Kk], torch.tensor([[-1, 2, 3], [Vs, 5, 6]]), ud)
    cdf = torch.cumsum(p[:, 0].double(), 1)
    want = [int((cdf[b] > float(ud[b, 1]) * float(cdf[b, -1])).int().argmax()) for b in range(2)]
    assert st["tokens"][:, 0].tolist() == want and st["cursor"].tolist() == [1, 1]
    # an eos in the middle of the accepted prefix stops there, emitted; the row is finished
    st = _verify(p, p[:, :Kk], d, u, eos=2, pad=7)
    assert st["cursor"].tolist() == [2, 4] and st["fin"].tolist() == [1, 0] and st["tokens"][0, :3].tolist() == [1, 2, -1]
    assert st["len"].tolist() == [7, 9]
    # cursor never passes N, and reaching it finishes the row
    st = _verify(p, p[:, :Kk], d, u, n=8, cursor=6)
    assert st["cursor"].tolist() == [8, 8] and st["fin"].tolist() == [1, 1] and st["len"].tolist() == [7, 7]
    assert torch.equal(st["tokens"][:, 6:], d[:, :2]) and st["counters"].tolist() == [4, 4]
    # a finished row emits nothing, keeps len and cursor, and gets padToken as its next input
    st = _verify(p, p[:, :Kk], d, u, pad=7, finished=[1, 0], cursor=3)
    assert st["cursor"].tolist() == [3, 7] and st["len"].tolist() == [5, 9] and st["fin"].tolist() == [1, 0]
    assert (st["tokens"][0] == -1).all() and int(st["next"][0]) == 7 and st["counters"].tolist() == [3, 3]
    # greedy: accept iff the draft is the argmax (lowest index among ties), the argmax is emitted at the rejection
    pg = torch.full((1, 2, 4), 0.1)
    pg[0, 0, 1] = pg[0, 0, 3] = 0.4
    pg[0, 1, 2] = 0.7
    z = torch.zeros(1, 4)
    st = _verify(pg, None, torch.tensor([[3]]), z, greedy=True)
    assert st["tokens"][0, :2].tolist() == [1, -1] and st["counters"].tolist() == [1, 0]
    st = _verify(pg, None, torch.tensor([[1]]), z, greedy=True)
    assert st["tokens"][0, :3].tolist() == [1, 2, -1] and st["counters"].tolist() == [1, 1]


def test_commit_twin():
    length = torch.tensor([7, 9, 4], dtype=torch.int32)
    short, slot = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    GN.spec_commit_torch(length, torch.tensor([0, 1, 0], dtype=torch.uint8), short, slot)
    assert short.tolist() == [2, 0, 5] and slot.tolist() == [2, 9]


# ------------------------------------------------------------------------------------------------ n-gram draft
NGRAM_CASES = [
    # (history up to and including the token not yet fed, ngram, K, drafts, what)
    ([1, 2, 3, 9, 1, 2, 3, 8, 1, 2, 3], 3, 4, [8, 1, 2, 3], "the latest of several matches wins; periodic extension"),
    ([1, 2, 3, 9, 1, 2, 3, 8, 1, 2, 3], 3, 2, [8, 1], "K shorter than the continuation"),
    ([5, 6, 7, 4, 4, 4, 1, 7], 3, 3, [4, 4, 4], "fallback from n = 3 to 1"),
    ([5, 6, 7, 8], 3, 3, [8, 8, 8], "no match: the last token"),
    ([3], 3, 2, [3, 3], "a history of one token"),
    ([2, 7, 7], 2, 3, [7, 7, 7], "a match that ends at the last fed token: period 1"),
    ([4, 5, 4, 5, 4, 5], 2, 5, [4, 5, 4, 5, 4], "overlapping match, period 2"),
    ([1, 2, 1, 2, 3, 1, 2], 8, 3, [3, 1, 2], "n larger than the history falls through to a shorter one"),
]


def test_ngram_draft_twin_on_hand_built_histories():
    for h, n, k, want, what in NGRAM_CASES:
        hist = torch.full((1, len(h) + 3), -7, dtype=torch.int64)
        hist[0, :len(h)] = torch.tensor(h)
        buf = torch.zeros(1, k + 1, dtype=torch.int64)
        GN.ngram_draft_torch(hist, torch.tensor([len(h) - 1], dtype=torch.int32), n, k, buf[:, 1:])
        assert buf[0, 1:].tolist() == want and int(buf[0, 0]) == 0, what


# ------------------------------------------------------------------------------------------------ rnnSetPositions
def _chunks():
    g = torch.Generator().manual_seed(2)
    return [torch.randint(0, V, s, generator=g) for s in ((3, 5), (3, 4), (3, 4))]


def _survivors(a, b, alen, keep):
    rows = [torch.cat([a[r, :alen[r]], b[r, :keep[r]]]) for r in range(3)]
    lens = torch.tensor([len(r) for r in rows])
    out = torch.zeros(3, int(lens.max()), dtype=torch.int64)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out, lens


@pytest.mark.parametrize("trimmed", [False, True])
def test_set_positions_equals_a_fresh_network_on_the_surviving_tokens(lms, trimmed):
    net, fresh = lms["net"], lms["copy"]
    a, b, c = _chunks()
    alen = [5, 3, 4] if trimmed else [5, 5, 5]
    net.rnnClearPreviousState()
    net.rnnTimeStep(a)
    if trimmed:
        net.rnnTrimState(torch.tensor(alen))
    net.rnnTimeStep(b)
    back = [0, 2, 3]
    lens = torch.tensor([alen[r] + 4 - back[r] for r in range(3)])
    bound = int(lens.max())
    short = (bound - lens).to(torch.int32)
    net.rnnSetPositions(bound, short)
    got = net.rnnTimeStep(c)
    st = net.rnnGetPreviousState(1)                              # the ordinary ragged state
    assert st["kv"].shape[1] == bound + 4 and torch.equal(st["short"], short)
    surv, slens = _survivors(a, b, alen, [4 - x for x in back])
    assert torch.equal(slens, lens)
    fresh.rnnClearPreviousState()
    fresh.rnnTimeStep(surv)
    fresh.rnnTrimState(slens)
    want = fresh.rnnTimeStep(c)
    assert float((got - want).abs().max()) <= 1e-12
    # the tensor is shared, not copied: an in-place update moves every layer
    assert all(l._kv_short is short for l in net.layers if hasattr(l, "_kv_short") and l._kv is not None)
    net.rnnClearPreviousState()
    assert all(getattr(l, "_kv_short", None) is None and getattr(l, "_short", None) is None for l in net.layers)


def test_set_positions_refusals(lms):
    net = lms["net"]
    a, b, _ = _chunks()
    short = torch.zeros(3, dtype=torch.int32)
    net.rnnClearPreviousState()
    net.rnnSetPositions(1, short)                                # no layer holds state: nothing to do
    net.rnnTimeStep(a)
    before = [(l._kv_len, l._kv_short) for l in net.layers if hasattr(l, "_kv_len")]
    for bound, sh, what in ((6, short, "1..5"), (0, short, "1..5"), (3, short.long(), "int32"),
                            (3, torch.zeros(2, dtype=torch.int32), "int32"),
                            (3, torch.zeros(3, 1, dtype=torch.int32), "int32"), (3, [0, 0, 0], "int32")):
        with pytest.raises(DL4JInvalidInputException, match=what):
            net.rnnSetPositions(bound, sh)
    assert [(l._kv_len, l._kv_short) for l in net.layers if hasattr(l, "_kv_len")] == before
    net.rnnPinState(12)
    with pytest.raises(DL4JInvalidInputException, match="pinned"):
        net.rnnSetPositions(3, short)
    net.rnnClearPreviousState()


def test_set_positions_names_an_lstm_layer_and_changes_nothing():
    net = TextGenerationLSTM(numLabels=11, seed=3, inputShape=[1, 11], hidden=16, dataType=DataType.DOUBLE).init(device=CPU)
    net.rnnClearPreviousState()
    net.rnnTimeStep(torch.nn.functional.one_hot(torch.tensor([[1, 2, 3]]), 11).permute(0, 2, 1).double())
    before = {k: v.clone() for k, v in net.rnnGetPreviousState(0).items() if torch.is_tensor(v)}
    with pytest.raises(DL4JInvalidInputException, match=r"layer 0: rnnSetPositions on layer 0 \(\w*LSTM\w*\)"):
        net.rnnSetPositions(2, torch.zeros(1, dtype=torch.int32))
    after = net.rnnGetPreviousState(0)
    assert before and all(torch.equal(v, after[k]) for k, v in before.items())


def test_set_positions_on_a_graph_with_input():
    net, fresh = _s2s(), _s2s()
    a, b, c = _chunks()
    g = torch.Generator().manual_seed(4)
    src = torch.randint(0, V, (3, 6), generator=g)
    net.rnnClearPreviousState()
    net.rnnTimeStep(src, a)
    net.rnnTimeStep(None, b)
    lens = torch.tensor([9, 7, 6])
    short = (9 - lens).to(torch.int32)
    with pytest.raises(DL4JInvalidInputException, match="network inputs"):
        net.rnnSetPositions(9, short, "nope")
    net.rnnSetPositions(9, short, "target")
    got = net.rnnTimeStep(None, c)[0]
    surv, slens = _survivors(a, b, [5, 5, 5], [4, 2, 1])
    fresh.rnnClearPreviousState()
    fresh.rnnTimeStep(src, surv)
    fresh.rnnTrimState(slens, "target")
    want = fresh.rnnTimeStep(None, c)[0]
    assert float((got - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ refusals
def test_speculative_refusals(lms):
    net, other = lms["net"], lms["other"]

    def refused(exc, match, assistant=None, **kw):
        net.rnnClearPreviousState()
        with pytest.raises(exc, match=match):
            net.generate(PROMPT, assistant=assistant, **kw)
        assert net.layers[1]._kv is None, "refused only after the prompt ran"

    refused(DL4JInvalidConfigException, "numDraftTokens", assistant=other)
    refused(DL4JInvalidConfigException, "numDraftTokens must be in 0..16", numDraftTokens=17)
    refused(DL4JInvalidConfigException, "draftNgram", numDraftTokens=2, draftNgram=9)
    refused(DL4JInvalidConfigException, "numBeams", numDraftTokens=2, numBeams=2)
    refused(DL4JInvalidConfigException, "useGraph", numDraftTokens=2, useGraph=True)
    refused(DL4JInvalidConfigException, "pinPositions", numDraftTokens=2, pinPositions=True)
    refused(DL4JInvalidConfigException, "topK", numDraftTokens=2, doSample=True, topK=5)
    refused(DL4JInvalidConfigException, "topP", numDraftTokens=2, doSample=True, topP=0.9)
    refused(DL4JInvalidInputException, "vocabulary", assistant=_lm(layers=1, vocab=V + 1), numDraftTokens=2)
    refused(DL4JInvalidInputException, "network of its own", assistant=net, numDraftTokens=2)
    lstm = TextGenerationLSTM(numLabels=V, seed=3, inputShape=[1, V], hidden=16, dataType=DataType.DOUBLE).init(device=CPU)
    refused(DL4JInvalidInputException, r"the assistant: layer 0: rnnSetPositions on layer 0 \(\w*LSTM", assistant=lstm,
            numDraftTokens=2, inputEncoding="ids")
    # 6 + 55 + 3 = 64 positions fit the table of 64, one more token does not; nor a shorter table of the assistant's
    net.generate(PROMPT, maxNewTokens=55, numDraftTokens=3)
    refused(DL4JInvalidInputException, "the network holds 64 positions", numDraftTokens=3, maxNewTokens=56)
    refused(DL4JInvalidInputException, "the assistant holds 32 positions", numDraftTokens=3, maxNewTokens=24,
            assistant=_lm(layers=1, maxPositions=32))
    with pytest.raises(DL4JInvalidInputException, match="LSTM"):
        lstm.generate(torch.tensor([[1, 2, 3]]), numDraftTokens=2, inputEncoding="onehot")
