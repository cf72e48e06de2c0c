"""Ragged prompts on the CPU: right-padded chunks through rnnTimeStep, ``rnnTrimState(lengths)`` and per-row
positions in the key/value caches and the position embedding (the torch paths that pin what the gfx950 kernels of
csrc/attention_decode.hip and csrc/nn_misc.hip must compute, tests/test_gpu_ragged_decode.py), ``generate`` with
``promptLengths`` / ``startLengths`` against one call per row, the refusals and the stored state."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidInputException
from deeplearning4j_amd.models import TransformerSeq2Seq

CPU = torch.device("cpu")
V, E = 11, 16
TP, LENS, STEPS = 9, (9, 1, 5, 8), 4


def _lm_layers(b):
    b.layer(0, BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(40).inputLength(TP).build())
    for i in (1, 2):
        b.layer(i, TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(2).ffnSize(24).causal(True).build())
    b.layer(3, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V).build())
    return b


@functools.lru_cache(maxsize=None)
def _mln(dt):
    b = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.3)).list())
    net = MultiLayerNetwork(_lm_layers(b).build())
    net.init(device=CPU)
    return net


@functools.lru_cache(maxsize=None)
def _graph(dt):
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.3)).graphBuilder())
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(40).inputLength(TP).build(), "tokens")
    prev = "emb"
    for i in range(2):
        g.addLayer(f"enc{i}", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(2).ffnSize(24).causal(True)
                   .build(), prev)
        prev = f"enc{i}"
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V)
               .build(), prev)
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device=CPU)
    return net


@functools.lru_cache(maxsize=None)
def _s2s():
    return TransformerSeq2Seq(numLabels=V, hidden=E, layers=2, heads=2, inputShape=[6, 16], maxPositions=40, seed=6,
                              dataType=DataType.DOUBLE).init(device=CPU)


def _tokens(seed=0):
    """(padded prompt [4, TP] with junk past every row's length, the teacher-forced continuation [4, STEPS])."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (len(LENS), TP), generator=g), torch.randint(0, V, (len(LENS), STEPS), generator=g)


def _step(net, x):
    out = net.rnnTimeStep(x)
    return out[0] if isinstance(out, list) else out


def _ragged_run(net, prompt, cont, lens):
    """Prefill on the padded rectangle, trim, teacher-forced steps -> per row [V, 1 + STEPS]: the distribution after
    the row's own last prompt token, then after every forced token."""
    net.rnnClearPreviousState()
    first = _step(net, prompt)
    net.rnnTrimState(torch.tensor(lens))
    outs = [torch.stack([first[b, :, n - 1] for b, n in enumerate(lens)])[:, :, None]]
    outs += [_step(net, cont[:, t:t + 1]) for t in range(cont.shape[1])]
    return torch.cat(outs, 2)


def _alone_run(net, prompt, cont, lens):
    rows = []
    for b, n in enumerate(lens):
        net.rnnClearPreviousState()
        outs = [_step(net, prompt[b:b + 1, :n])[:, :, -1:]]
        outs += [_step(net, cont[b:b + 1, t:t + 1]) for t in range(cont.shape[1])]
        rows.append(torch.cat(outs, 2))
    net.rnnClearPreviousState()
    return torch.cat(rows, 0)


# ------------------------------------------------------------------------------------------------ layer path
@pytest.mark.parametrize("make", [_mln, _graph], ids=["MultiLayerNetwork", "ComputationGraph"])
@pytest.mark.parametrize("dt", [DataType.FLOAT, DataType.DOUBLE], ids=["fp32", "fp64"])
def test_trimmed_rows_continue_like_the_row_alone(make, dt):
    net = make(dt)
    prompt, cont = _tokens()
    got = _ragged_run(net, prompt, cont, LENS)
    want = _alone_run(net, prompt, cont, LENS)
    err = (got.double() - want.double()).abs().max().item()
    print(f"ragged vs alone {dt}: max abs err {err:.3e}")
    assert got.shape == (4, V, 1 + STEPS)
    assert err < 1e-4
    # the padding is junk the valid rows never see: other junk, same result
    other = prompt.clone()
    for b, n in enumerate(LENS):
        other[b, n:] = (other[b, n:] + 3) % V
    assert torch.equal(_ragged_run(net, other, cont, LENS), got)
    net.rnnClearPreviousState()


def test_untrimmed_padding_is_what_goes_wrong():
    """The control: without the trim the padded rows continue at the common position and differ from the row alone."""
    net = _graph(DataType.DOUBLE)
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    _step(net, prompt)
    got = _step(net, cont[:, :1])
    want = _alone_run(net, prompt, cont, LENS)[:, :, 1:2]
    assert (got[0] - want[0]).abs().max() < 1e-9                 # the full-length row
    assert (got[1] - want[1]).abs().max() > 1e-4                 # the one-token row
    net.rnnClearPreviousState()


# ------------------------------------------------------------------------------------------------ generate
def _per_row(net, prompt, lens, **kw):
    rs = [net.generate(prompt[b:b + 1, :n], **kw) for b, n in enumerate(lens)]
    return (torch.cat([r.tokens for r in rs]), torch.cat([r.lengths for r in rs]), torch.cat([r.scores for r in rs]))


@pytest.mark.parametrize("kw", [dict(), dict(numBeams=3), dict(eosToken=3, padToken=0),
                                dict(numBeams=3, eosToken=3, padToken=0)], ids=["greedy", "beam", "greedy-eos",
                                                                                "beam-eos"])
def test_generate_with_prompt_lengths_equals_one_call_per_row(kw):
    net = _graph(DataType.DOUBLE)
    prompt, _ = _tokens(1)
    r = net.generate(prompt, promptLengths=LENS, maxNewTokens=6, **kw)
    tokens, lengths, scores = _per_row(net, prompt, LENS, maxNewTokens=6, **kw)
    assert torch.equal(r.tokens, tokens) and torch.equal(r.lengths, lengths)
    assert (r.scores.double() - scores.double()).abs().max() < 1e-9
    other = prompt.clone()
    for b, n in enumerate(LENS):
        other[b, n:] = (other[b, n:] + 5) % V
    o = net.generate(other, promptLengths=torch.tensor(LENS), maxNewTokens=6, **kw)
    assert torch.equal(o.tokens, r.tokens) and torch.equal(o.lengths, r.lengths) and torch.equal(o.scores, r.scores)


@pytest.mark.parametrize("kw", [dict(), dict(numBeams=3)], ids=["greedy", "beam"])
def test_equal_lengths_are_the_call_without_lengths(kw):
    net = _mln(DataType.DOUBLE)
    prompt, _ = _tokens(2)
    a = net.generate(prompt, maxNewTokens=5, **kw)
    b = net.generate(prompt, promptLengths=[TP] * 4, maxNewTokens=5, **kw)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.scores, b.scores)


@pytest.mark.parametrize("kw", [dict(), dict(numBeams=3)], ids=["greedy", "beam"])
def test_seq2seq_start_lengths_equal_one_call_per_row(kw):
    net = _s2s()
    g = torch.Generator().manual_seed(3)
    source = torch.randint(0, V, (3, 6), generator=g)
    smask = torch.tensor([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0]], dtype=torch.float32)
    start = torch.randint(0, V, (3, 4), generator=g)
    lens = (2, 4, 1)
    r = TransformerSeq2Seq.generate(net, source, start, sourceMask=smask, startLengths=lens, maxNewTokens=5, **kw)
    # the encoder side was fed 6 source tokens per row and is not trimmed by the target's lengths
    assert "short" not in net.rnnGetPreviousState("source_embeddings")
    assert "short" in net.rnnGetPreviousState("target_embeddings")
    assert "short" in net.rnnGetPreviousState("decoder_0") and "mem_kv" in net.rnnGetPreviousState("decoder_0")
    for b, n in enumerate(lens):
        one = TransformerSeq2Seq.generate(net, source[b:b + 1], start[b:b + 1, :n], sourceMask=smask[b:b + 1],
                                          maxNewTokens=5, **kw)
        assert torch.equal(r.tokens[b:b + 1], one.tokens) and torch.equal(r.lengths[b:b + 1], one.lengths)
        assert (r.scores[b:b + 1].double() - one.scores.double()).abs().max() < 1e-9


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("lens", [(9, 0, 5, 8), (9, 1, 10, 8), (9, 1, 5), (9.0, 1.0, 5.0, 8.0), (-1, 1, 5, 8)])
def test_lengths_out_of_range_are_refused_and_change_nothing(lens):
    net = _graph(DataType.FLOAT)
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    _step(net, prompt)
    with pytest.raises(DL4JInvalidInputException, match="rnnTrimState"):
        net.rnnTrimState(torch.tensor(lens))
    assert all("short" not in net.rnnGetPreviousState(n) for n in ("emb", "enc0", "enc1"))
    net.rnnTrimState(LENS)                                       # still possible: nothing was trimmed
    net.rnnClearPreviousState()


def test_trim_before_any_step_is_refused():
    net = _graph(DataType.FLOAT)
    net.rnnClearPreviousState()
    with pytest.raises(DL4JInvalidInputException, match="rnnTrimState"):
        net.rnnTrimState([1, 1])


def test_a_second_trim_is_refused_until_the_state_is_cleared():
    net = _mln(DataType.FLOAT)
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnTrimState(LENS)
    before = net.rnnGetPreviousState(1)["short"].clone()
    with pytest.raises(DL4JInvalidInputException, match="trimmed already"):
        net.rnnTrimState(LENS)
    _step(net, cont[:, :1])
    with pytest.raises(DL4JInvalidInputException, match="trimmed already"):
        net.rnnTrimState((1, 1, 1, 1))
    assert torch.equal(net.rnnGetPreviousState(1)["short"], before)
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnTrimState(LENS)
    net.rnnClearPreviousState()


def _lstm_net(wrapped):
    b = (NeuralNetConfiguration.Builder().seed(3).dataType(DataType.FLOAT).updater(NoOp()).list())
    b.layer(0, SelfAttentionLayer.Builder().nIn(V).nOut(8).nHeads(2).causal(True).activation(Activation.IDENTITY)
            .build())
    lstm = LSTM.Builder().nIn(8).nOut(8).activation(Activation.TANH).build()
    b.layer(1, MaskZeroLayer(underlying=lstm, maskingValue=0.0) if wrapped else lstm)
    b.layer(2, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(8).nOut(V).build())
    net = MultiLayerNetwork(b.build())
    net.init(device=CPU)
    return net


def test_a_network_with_an_lstm_is_refused_and_left_as_it_was():
    net = _lstm_net(False)
    x = torch.randn(2, V, 5, generator=torch.Generator().manual_seed(0))
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    kv = net.rnnGetPreviousState(0)
    h = {k: v.clone() for k, v in net.rnnGetPreviousState(1).items() if torch.is_tensor(v)}
    with pytest.raises(DL4JInvalidInputException, match=r"layer 1 \(LSTM\)"):
        net.rnnTrimState([5, 2])
    after = net.rnnGetPreviousState(0)
    assert set(after) == set(kv) == {"kv"} and torch.equal(after["kv"], kv["kv"])     # the attention layer before it
    now = net.rnnGetPreviousState(1)
    assert h and all(torch.equal(now[k], v) for k, v in h.items())
    nxt = torch.randn(2, V, 1, generator=torch.Generator().manual_seed(1))
    a = net.rnnTimeStep(nxt)
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    assert torch.equal(net.rnnTimeStep(nxt), a)                  # the refused call left no trace
    with pytest.raises(DL4JInvalidInputException, match="LSTM"):
        net.generate(torch.tensor([[1, 2, 3], [4, 5, 0]]), promptLengths=[3, 2], inputEncoding="onehot",
                     maxNewTokens=2)


def test_a_wrapper_forwards_the_trim_to_the_layer_it_wraps():
    net = _lstm_net(True)
    x = torch.randn(2, V, 5, generator=torch.Generator().manual_seed(0))
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    with pytest.raises(DL4JInvalidInputException, match=r"\(LSTM\)"):
        net.rnnTrimState([5, 2])
    assert "short" not in net.rnnGetPreviousState(0)


def test_invalid_prompt_lengths_are_refused_by_generate():
    net = _graph(DataType.FLOAT)
    prompt, _ = _tokens()
    for bad in [(9, 0, 5, 8), (9, 1, 5, 10), (9, 1, 5), (9.5, 1.0, 5.0, 8.0), "abcd"]:
        with pytest.raises(DL4JInvalidInputException, match="generate"):
            net.generate(prompt, promptLengths=bad, maxNewTokens=2)
    with pytest.raises(DL4JInvalidInputException, match="ragged prompts are not supported"):
        net.generate([[1, 2, 3], [4, 5]], maxNewTokens=2)       # a ragged list without lengths: as before


# ------------------------------------------------------------------------------------------------ stored state
def test_the_stored_state_round_trips_the_shortfall():
    net = _graph(DataType.DOUBLE)
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnTrimState(LENS)
    _step(net, cont[:, :1])
    want_short = torch.tensor([TP - n for n in LENS], dtype=torch.int32)
    states = net.rnnGetPreviousStates()
    for n in ("emb", "enc0", "enc1"):
        assert torch.equal(states[n]["short"], want_short) and states[n]["short"].dtype == torch.int32
    assert states["emb"]["pos"] == TP + 1 and states["enc0"]["kv"].shape == (4, TP + 1, 2 * E)
    a = _step(net, cont[:, 1:2])
    net.rnnClearPreviousState()
    assert net.rnnGetPreviousState("enc0") == {} and net.rnnGetPreviousState("emb") == {}
    net.rnnSetPreviousStates(states)
    again = net.rnnGetPreviousStates()
    for n in ("emb", "enc0", "enc1"):
        assert torch.equal(again[n]["short"], want_short)
    assert torch.equal(_step(net, cont[:, 1:2]), a)
    with pytest.raises(DL4JInvalidInputException, match="trimmed already"):
        net.rnnTrimState(LENS)                                   # a restored shortfall counts as a trim
    net.rnnClearPreviousState()


def test_reorder_permutes_the_shortfall_and_keeps_it_within_groups():
    net = _graph(DataType.DOUBLE)
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnTrimState(LENS)
    short = torch.tensor([TP - n for n in LENS], dtype=torch.int32)
    parents = torch.tensor([2, 2, 0, 3, 1, 1], dtype=torch.int32)
    net.rnnReorderState(parents)
    for n in ("emb", "enc0", "enc1"):
        assert torch.equal(net.rnnGetPreviousState(n)["short"], short[parents.long()])
    got = _step(net, cont[parents.long(), :1])
    want = _alone_run(net, prompt, cont, LENS)[:, :, 1:2]
    assert (got - want[parents.long()]).abs().max() < 1e-9
    # groups of 2 rows that share a prompt: parents within the group, same number of rows -> the array stays
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnTrimState(LENS)
    net.rnnReorderState(torch.arange(4, dtype=torch.int32).repeat_interleave(2))
    kept = net.rnnGetPreviousState("enc0")["short"].clone()
    net.rnnReorderState(torch.tensor([1, 0, 2, 2, 5, 5, 7, 6], dtype=torch.int32), groupSize=2)
    assert torch.equal(net.rnnGetPreviousState("enc0")["short"], kept)
    assert torch.equal(kept, short.repeat_interleave(2))
    net.rnnClearPreviousState()
