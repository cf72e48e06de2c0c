"""Token generation on the CPU (the torch paths of ops/generation_native.py): these pin the semantics the gfx950
kernels of csrc/generation.hip must match (tests/test_gpu_generation.py)."""
import itertools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.models import TextGenerationLSTM, TextGenerationTransformer, TransformerSeq2Seq
from deeplearning4j_amd.nn.generation import GenerationConfig
from deeplearning4j_amd.ops import generation_native as GN
from deeplearning4j_amd.ops.nn_misc import PhiloxStream

CPU = torch.device("cpu")


def _lm(V=11, hidden=32, layers=2, dt=DataType.FLOAT, device=CPU):
    return TextGenerationTransformer(numLabels=V, hidden=hidden, layers=layers, heads=2, inputShape=[16],
                                     maxPositions=64, seed=5, dataType=dt).init(device=device)


def _s2s(V=11, hidden=32, dt=DataType.FLOAT, device=CPU):
    return TransformerSeq2Seq(numLabels=V, hidden=hidden, layers=2, heads=2, inputShape=[8, 16], maxPositions=64,
                              seed=6, dataType=dt).init(device=device)


def _rng(seed, device=CPU):
    s = PhiloxStream(device)
    s.seed = seed
    return s


@pytest.fixture(scope="module")
def lm():
    return _lm()


PROMPT = torch.tensor([[1, 2, 3], [4, 5, 6], [7, 0, 9]])


def _greedy_by_output(net, prompt, n):
    seq = prompt.clone()
    logp = torch.zeros(prompt.shape[0], dtype=torch.float64)
    for _ in range(n):
        p = net.output(seq)[0][:, :, -1]
        nxt = p.argmax(1)
        logp += torch.log(p.double().gather(1, nxt[:, None]))[:, 0]
        seq = torch.cat([seq, nxt[:, None]], 1)
    return seq[:, prompt.shape[1]:], logp


# ------------------------------------------------------------------------------------------------ 1, 2: greedy
def test_greedy_equals_argmax_of_output_on_the_growing_sequence(lm):
    r = lm.generate(PROMPT, maxNewTokens=6)
    want, logp = _greedy_by_output(lm, PROMPT, 6)
    assert r.tokens.dtype == torch.int64 and torch.equal(r.tokens, want)
    assert torch.equal(r.lengths, torch.full((3,), 6))
    assert (r.scores.double() - logp).abs().max() < 1e-4
    again = TextGenerationTransformer.generate(lm, PROMPT, maxNewTokens=6)
    assert torch.equal(again.tokens, want)


def test_beam_width_one_equals_greedy(lm):
    g = lm.generate(PROMPT, maxNewTokens=6, lengthPenalty=0.0)
    b = lm.generate(PROMPT, maxNewTokens=6, lengthPenalty=0.0, useBeamPath=True)
    assert torch.equal(g.tokens, b.tokens) and torch.equal(g.lengths, b.lengths)
    assert (g.scores - b.scores).abs().max() < 1e-5


# ------------------------------------------------------------------------------------------------ 3: exhaustive
def test_full_width_beam_search_finds_the_best_of_all_continuations():
    net = _lm(V=4, hidden=32, layers=1)
    prompt = torch.tensor([[1, 2], [3, 0]])
    r = net.generate(prompt, maxNewTokens=3, numBeams=16, lengthPenalty=0.0)
    conts = torch.tensor(list(itertools.product(range(4), repeat=3)))              # [64, 3]
    for b in range(2):
        seqs = torch.cat([prompt[b].expand(64, 2), conts], 1)
        p = net.output(seqs)[0].double()                                           # [64, 4, 5]
        lp = sum(torch.log(p[torch.arange(64), conts[:, j], 1 + j]) for j in range(3))
        best = int(lp.argmax())
        assert torch.equal(r.tokens[b], conts[best]), (r.tokens[b], conts[best])
        assert abs(float(r.scores[b]) - float(lp[best])) < 1e-5
    assert torch.equal(r.lengths, torch.tensor([3, 3]))


# ------------------------------------------------------------------------------------------------ 4: end of sequence
@pytest.mark.parametrize("mode", ["greedy", "sample", "beam"])
def test_eos_pads_counts_and_does_not_depend_on_the_check_interval(lm, mode):
    kw = {"greedy": {}, "sample": dict(doSample=True, seed=9, topK=6), "beam": dict(numBeams=3)}[mode]
    free = lm.generate(PROMPT, maxNewTokens=10, **kw).tokens
    eos = int(free[0, 2])                                        # row 0 meets it at step 2 at the latest
    pad = (eos + 1) % 11
    rs = [lm.generate(PROMPT, maxNewTokens=10, eosToken=eos, padToken=pad, eosCheckEvery=e, **kw)
          for e in (1, 3, 1000)]
    r = rs[0]
    for o in rs[1:]:
        assert torch.equal(o.tokens, r.tokens) and torch.equal(o.lengths, r.lengths)
        assert torch.equal(o.scores, r.scores)
    assert int(r.lengths[0]) <= 3
    for b in range(3):
        row, n = r.tokens[b], int(r.lengths[b])
        hits = (row == eos).nonzero()
        if len(hits):
            assert n == int(hits[0]) + 1
            assert (row[n:] == pad).all()
        else:
            assert n == 10


# ------------------------------------------------------------------------------------------------ 5: reorder
PARENTS = [2, 0, 0, 1]          # a permutation, a duplicate and an expansion 3 -> 4 at once


def _float_steps(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, n, 5, generator=g), torch.randn(4, n, 1, generator=g)


def _sa_net():
    b = (NeuralNetConfiguration.Builder().seed(11).dataType(DataType.FLOAT).updater(NoOp())
         .weightInit(NormalDistribution(0, 0.2)).list())
    b.layer(0, SelfAttentionLayer.Builder().nIn(16).nOut(16).nHeads(2).causal(True)
            .activation(Activation.IDENTITY).build())
    b.layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).nIn(16).nOut(5).activation(Activation.SOFTMAX).build())
    net = MultiLayerNetwork(b.build())
    net.init(device=CPU)
    return net


def _dec_graph():
    g = (NeuralNetConfiguration.Builder().seed(3).dataType(DataType.FLOAT).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.2)).graphBuilder())
    g.addInputs("mem", "x")
    g.addLayer("dec", TransformerDecoderLayer.Builder().nIn(16).nInMemory(16).nOut(16).nHeads(2).ffnSize(24).build(),
               "x", "mem")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(16).nOut(5)
               .build(), "dec")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device=CPU)
    return net


def _out(o):
    return o[0] if isinstance(o, (list, tuple)) else o


@pytest.mark.parametrize("kind", ["encoder", "selfattention", "decoder", "lstm"])
def test_reorder_state_equals_a_fresh_network_on_the_selected_rows(kind):
    idx = torch.tensor(PARENTS)
    if kind == "encoder":
        net = _lm()
        a = torch.randint(0, 11, (3, 5), generator=torch.Generator().manual_seed(1))
        b = torch.randint(0, 11, (4, 1), generator=torch.Generator().manual_seed(2))
        first = lambda rows: (a[rows],)                                            # noqa: E731
        nxt, kw = (b,), {}
    elif kind == "selfattention":
        net = _sa_net()
        a, b = _float_steps(16, 4)
        first = lambda rows: (a[rows],)                                            # noqa: E731
        nxt, kw = (b,), {}
    elif kind == "decoder":
        net = _dec_graph()
        a, b = _float_steps(16, 5)
        mem = torch.randn(3, 16, 4, generator=torch.Generator().manual_seed(6))
        mmask = torch.tensor([[1., 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]])
        first = lambda rows: (mem[rows], a[rows])                                  # noqa: E731
        nxt = (None, b)
        kw = lambda rows: dict(masks=[mmask[rows], None])                          # noqa: E731
    else:
        net = TextGenerationLSTM(numLabels=7, inputShape=[1, 7], hidden=8, seed=2).init(device=CPU)
        g = torch.Generator().manual_seed(8)
        a = torch.nn.functional.one_hot(torch.randint(0, 7, (3, 5), generator=g), 7).permute(0, 2, 1).float()
        b = torch.nn.functional.one_hot(torch.randint(0, 7, (4, 1), generator=g), 7).permute(0, 2, 1).float()
        first = lambda rows: (a[rows],)                                            # noqa: E731
        nxt, kw = (b,), {}
    kwf = kw if callable(kw) else (lambda rows: {})
    net.rnnClearPreviousState()
    net.rnnTimeStep(*first(torch.arange(3)), **kwf(torch.arange(3)))
    net.rnnReorderState(torch.tensor(PARENTS, dtype=torch.int32))
    got = _out(net.rnnTimeStep(*nxt))
    net.rnnClearPreviousState()
    net.rnnTimeStep(*first(idx), **kwf(idx))
    want = _out(net.rnnTimeStep(*nxt))
    assert got.shape[0] == 4 and torch.allclose(got, want, atol=1e-6, rtol=1e-5)
    # and it is not the unpermuted state
    net.rnnClearPreviousState()
    net.rnnTimeStep(*first(torch.tensor([0, 1, 2, 0])), **kwf(torch.tensor([0, 1, 2, 0])))
    assert not torch.allclose(_out(net.rnnTimeStep(*nxt)), want, atol=1e-6)


@pytest.mark.parametrize("grouped", [False, True])
def test_reorder_state_seq2seq_with_and_without_group_size(grouped):
    net = _s2s()
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 11, (2, 6), generator=g)
    smask = torch.tensor([[1., 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    start = torch.randint(0, 11, (2, 3), generator=g)
    t1 = torch.randint(0, 11, (4, 1), generator=g)
    t2 = torch.randint(0, 11, (4, 1), generator=g)
    expand, perm = torch.tensor([0, 0, 1, 1]), torch.tensor([1, 0, 3, 3])
    net.rnnClearPreviousState()
    net.rnnTimeStep(src, start, masks=[smask, None])
    net.rnnReorderState(expand.int())
    net.rnnTimeStep(None, t1)
    net.rnnReorderState(perm.int(), groupSize=2 if grouped else None)
    got = net.rnnTimeStep(None, t2)[0]
    rows = expand[perm]
    net.rnnClearPreviousState()
    net.rnnTimeStep(src[rows], start[rows], masks=[smask[rows], None])
    net.rnnTimeStep(None, t1[perm])
    want = net.rnnTimeStep(None, t2)[0]
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-5)


def test_seq2seq_and_lstm_generate():
    net = _s2s()
    g = torch.Generator().manual_seed(4)
    src = torch.randint(0, 11, (2, 6), generator=g)
    smask = torch.tensor([[1., 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    start = torch.tensor([[1], [1]])
    r = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=4, lengthPenalty=0.0)
    seq = start.clone()
    for _ in range(4):
        p = net.output(src, seq, masks=[smask, None])[0][:, :, -1]
        seq = torch.cat([seq, p.argmax(1)[:, None]], 1)
    assert torch.equal(r.tokens, seq[:, 1:])
    b = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=4, numBeams=4, lengthPenalty=0.0)
    assert (b.scores >= r.scores - 1e-5).all()
    lstm = TextGenerationLSTM(numLabels=7, inputShape=[1, 7], hidden=8, seed=2).init(device=CPU)
    pr = torch.tensor([[1, 2, 3], [4, 5, 6]])
    rl = TextGenerationLSTM.generate(lstm, pr, maxNewTokens=4, lengthPenalty=0.0)
    seq = pr.clone()
    for _ in range(4):
        x = torch.nn.functional.one_hot(seq, 7).permute(0, 2, 1).float()
        seq = torch.cat([seq, lstm.output(x)[:, :, -1].argmax(1)[:, None]], 1)
    assert torch.equal(rl.tokens, seq[:, 3:])
    bl = TextGenerationLSTM.generate(lstm, pr, maxNewTokens=4, numBeams=3, lengthPenalty=0.0)
    assert (bl.scores >= rl.scores - 1e-5).all()


# ------------------------------------------------------------------------------------------------ 6: sampling
def test_kept_set_oracle_on_a_hand_computed_row():
    p = torch.tensor([[0.5, 0.2, 0.2, 0.1]])
    ks = lambda **kw: GN.sample_kept_set(p, **kw)[0][0].tolist()                  # noqa: E731
    assert ks() == [True] * 4
    assert ks(topK=1) == [True, False, False, False]
    assert ks(topK=2) == [True, True, True, False]               # the tie at the 2nd largest value is kept whole
    assert ks(topK=4) == [True] * 4 and ks(topK=7) == [True] * 4
    assert ks(topP=0.45) == [True, False, False, False]
    assert ks(topP=0.6) == [True, True, True, False]
    assert ks(topP=0.95) == [True] * 4
    assert ks(topP=1e-6) == [True, False, False, False]
    assert ks(topK=2, topP=0.99) == [True, True, True, False]    # top-p among the top-k survivors


V6 = 8


def _rows6():
    g = torch.Generator().manual_seed(12)
    rand = torch.softmax(2.0 * torch.randn(V6, generator=g), 0)
    tied = rand.clone()
    tied[3] = tied[5] = tied.max()                               # tied maxima
    tied = tied / tied.sum()
    equal = torch.full((V6,), 1.0 / V6)
    onehot = torch.zeros(V6)
    onehot[6] = 1.0
    return {"random": rand, "tiedmax": tied, "equal": equal, "onehot": onehot}


@pytest.mark.parametrize("topK", [0, 1, 2, V6, V6 + 3])
@pytest.mark.parametrize("topP", [1.0, 0.9, 1e-6])
def test_sampler_draws_exactly_from_the_kept_set(topK, topP):
    for name, row in _rows6().items():
        p = row.reshape(1, V6).repeat(256, 1)
        keep = GN.sample_kept_set(p[:1], 1.0, topK, topP)[0][0]
        tok, logp, u = GN.sample_rows_torch(p, 1.0, topK, topP, False, _rng(77))
        assert torch.equal(u, GN.sample_uniform(77, 0, 256))
        drawn = torch.zeros(V6, dtype=torch.bool)
        drawn[tok] = True
        assert not (drawn & ~keep).any(), (name, topK, topP, drawn, keep)
        assert torch.allclose(logp, torch.log(p[torch.arange(256), tok]))
        if name == "equal":
            assert keep.all() and drawn.all()                    # ties all kept (and 256 draws reach all 8)
        if name == "onehot":
            assert drawn.tolist() == [i == 6 for i in range(V6)]     # zeros never drawn
        if topP == 1e-6 or topK == 1:
            assert torch.equal(keep, row == row.max()), (name, keep)   # only the maximum, or all tied maxima
            if name == "tiedmax":
                assert int(keep.sum()) == 3 and torch.equal(drawn, keep)


def test_sampling_is_a_function_of_the_seed(lm):
    p = torch.softmax(torch.randn(256, 50, generator=torch.Generator().manual_seed(1)), 1)
    a = GN.sample_rows_torch(p, 0.9, 0, 1.0, False, _rng(5))[0]
    b = GN.sample_rows_torch(p, 0.9, 0, 1.0, False, _rng(5))[0]
    c = GN.sample_rows_torch(p, 0.9, 0, 1.0, False, _rng(6))[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
    kw = dict(maxNewTokens=8, doSample=True, temperature=1.5)
    r1, r2, r3 = (lm.generate(PROMPT, seed=s, **kw).tokens for s in (21, 21, 22))
    assert torch.equal(r1, r2) and not torch.equal(r1, r3)
    torch.manual_seed(3)
    u1 = lm.generate(PROMPT, **kw).tokens
    torch.manual_seed(3)
    u2 = lm.generate(PROMPT, **kw).tokens
    assert torch.equal(u1, u2)                                   # seed=None: from torch's generator


def test_greedy_flag_takes_the_lowest_index_among_tied_maxima():
    p = torch.tensor([[0.1, 0.3, 0.3, 0.3], [0.25, 0.25, 0.25, 0.25]])
    tok, logp, _ = GN.sample_rows_torch(p, greedy=True)
    assert tok.tolist() == [1, 0] and torch.allclose(logp, torch.log(torch.tensor([0.3, 0.25])))


def test_beam_step_torch_matches_the_reference():
    g = torch.Generator().manual_seed(2)
    for B, W, V in ((1, 1, 3), (3, 3, 3), (2, 8, 5), (3, 16, 77)):
        p = torch.softmax(torch.randn(B * W, V, generator=g), 1)
        p[0, 0] = 0.0
        score = torch.full((B, W), float("-inf"))
        score[:, 0] = 0.0
        fin = torch.zeros(B, W, dtype=torch.uint8)
        length = torch.zeros(B, W, dtype=torch.int32)
        for step in range(3):
            want = GN.beam_step_reference(p, score, fin, length, eosToken=1, padToken=2)
            par, tok = GN.beam_step_torch(p, score, fin, length, eosToken=1, padToken=2)
            assert torch.equal(par, want[0]) and torch.equal(tok, want[1]), (B, W, V, step)
            assert torch.allclose(score.double(), want[2], atol=1e-5)
            assert torch.equal(fin, want[3]) and torch.equal(length, want[4])
            p = torch.softmax(torch.randn(B * W, V, generator=g), 1)


# ------------------------------------------------------------------------------------------------ 7: validation
@pytest.mark.parametrize("kw", [dict(numBeams=0), dict(numBeams=17), dict(doSample=True, numBeams=2),
                                dict(temperature=0.0), dict(temperature=-1.0), dict(topP=0.0), dict(topP=1.5),
                                dict(topK=-1), dict(maxNewTokens=0), dict(inputEncoding="bytes"),
                                dict(eosCheckEvery=0), dict(noSuchField=1)])
def test_bad_config_values_are_refused(lm, kw):
    with pytest.raises(DL4JInvalidConfigException):
        lm.generate(PROMPT, **kw)


def test_config_object_and_keyword_overrides(lm):
    cfg = GenerationConfig(maxNewTokens=3)
    assert lm.generate(PROMPT, cfg).tokens.shape == (3, 3)
    assert lm.generate(PROMPT, cfg, maxNewTokens=5).tokens.shape == (3, 5)
    assert cfg.maxNewTokens == 3


def test_a_ragged_prompt_is_refused(lm):
    with pytest.raises(DL4JInvalidInputException, match="ragged"):
        lm.generate([[1, 2, 3], [4, 5]], maxNewTokens=2)
    with pytest.raises(DL4JInvalidInputException, match="ragged"):
        lm.generate(torch.tensor([1, 2, 3]), maxNewTokens=2)


def test_public_rnn_time_step_still_returns_fp32_and_states_are_unchanged(lm):
    lm.rnnClearPreviousState()
    out = lm.rnnTimeStep(PROMPT)[0]
    assert out.dtype == torch.float32 and out.shape == (3, 11, 3)
    assert lm.rnnGetPreviousState("decoder_0")["kv"].shape == (3, 3, 64)
