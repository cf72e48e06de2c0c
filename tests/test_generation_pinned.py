"""Pinned rnnTimeStep state on the CPU (the torch paths that take per-row shortfalls): ``rnnPinState`` fixes the host's
bound and lets one device array carry the positions, ``generate(pinPositions=True)`` runs on it and equals the ordinary
call, the stored state continues on another network, and everything that cannot work while pinned is refused."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.models import TransformerSeq2Seq
from deeplearning4j_amd.nn.generation import GenerationConfig

CPU = torch.device("cpu")
V, E, MAXP = 11, 16, 40
TP, LENS = 9, (9, 1, 5, 8)
SAMPLING = dict(doSample=True, temperature=0.8, topK=5, topP=0.9, seed=3)


def _lm_layers(b):
    b.layer(0, BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(MAXP).inputLength(TP).build())
    for i in (1, 2):
        b.layer(i, TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(2).ffnSize(24).causal(True).build())
    b.layer(3, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V).build())
    return b


def _new_mln(dt=DataType.DOUBLE):
    b = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.3)).list())
    net = MultiLayerNetwork(_lm_layers(b).build())
    net.init(device=CPU)
    return net


@functools.lru_cache(maxsize=None)
def _mln(dt=DataType.DOUBLE):
    return _new_mln(dt)


@functools.lru_cache(maxsize=None)
def _graph():
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(DataType.DOUBLE).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.3)).graphBuilder())
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(MAXP).inputLength(TP).build(), "tokens")
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
    return TransformerSeq2Seq(numLabels=V, hidden=E, layers=2, heads=2, inputShape=[6, 16], maxPositions=MAXP, seed=6,
                              dataType=DataType.DOUBLE).init(device=CPU)


def _tokens(seed=0, steps=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (len(LENS), TP), generator=g), torch.randint(0, V, (len(LENS), steps), generator=g)


def _step(net, x):
    out = net.rnnTimeStep(x)
    return out[0] if isinstance(out, list) else out


def _close(a, b):
    """Tokens and lengths exactly, scores within the row-alone tolerance of tests/test_ragged_generation.py."""
    return torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and \
        (a.scores.double() - b.scores.double()).abs().max() < 1e-9


# ------------------------------------------------------------------------------------------------ generate
@pytest.mark.parametrize("kw", [dict(), SAMPLING, dict(SAMPLING, eosToken=4, padToken=0, eosCheckEvery=2)],
                         ids=["greedy", "sampling", "sampling-eos"])
@pytest.mark.parametrize("make", [_mln, _graph], ids=["MultiLayerNetwork", "ComputationGraph"])
@pytest.mark.parametrize("lens", [None, LENS], ids=["uniform", "ragged"])
def test_pinned_generate_equals_the_ordinary_call(make, lens, kw):
    net = make()
    prompt, _ = _tokens(1)
    want = net.generate(prompt, promptLengths=lens, maxNewTokens=7, **kw)
    got = net.generate(prompt, promptLengths=lens, maxNewTokens=7, pinPositions=True, **kw)
    assert _close(got, want)
    st = net.lastGenerationStats
    assert st["captures"] == st["graphReplays"] == 0 and 1 <= st["eagerSteps"] <= 7
    assert "eosToken" in kw or st["eagerSteps"] == 7
    assert net._rnn_pin is not None and net._rnn_pin["record"] is None       # pinned still, the call's buffers gone
    net.rnnClearPreviousState()
    assert net._rnn_pin is None


def test_pinned_generate_seq2seq_with_a_mask_and_start_lengths():
    net = _s2s()
    g = torch.Generator().manual_seed(3)
    source = torch.randint(0, V, (3, 6), generator=g)
    smask = torch.tensor([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0]], dtype=torch.float32)
    start = torch.randint(0, V, (3, 4), generator=g)
    for lens in (None, (2, 4, 1)):
        want = TransformerSeq2Seq.generate(net, source, start, sourceMask=smask, startLengths=lens, maxNewTokens=6)
        got = TransformerSeq2Seq.generate(net, source, start, sourceMask=smask, startLengths=lens, maxNewTokens=6,
                                          pinPositions=True)
        assert _close(got, want)
        # the encoder side is not downstream of the target input: left alone
        assert not net.layers_by_name["source_embeddings"]._pinned
        assert net.layers_by_name["target_embeddings"]._pinned and net.layers_by_name["decoder_1"]._kv_pinned
    net.rnnClearPreviousState()


def test_one_token_and_a_full_position_table():
    net = _mln()
    prompt, _ = _tokens(2)
    assert _close(net.generate(prompt, maxNewTokens=1, pinPositions=True), net.generate(prompt, maxNewTokens=1))
    n = MAXP - TP + 1                                            # the last token is sampled, never fed: it still fits
    assert _close(net.generate(prompt, maxNewTokens=n, pinPositions=True), net.generate(prompt, maxNewTokens=n))
    with pytest.raises(DL4JInvalidInputException, match="maxPositions"):
        net.generate(prompt, maxNewTokens=n + 1, pinPositions=True)
    net.rnnClearPreviousState()


# ------------------------------------------------------------------------------------------------ by hand
@pytest.mark.parametrize("make", [_mln, _graph], ids=["MultiLayerNetwork", "ComputationGraph"])
@pytest.mark.parametrize("lens", [None, LENS], ids=["uniform", "ragged"])
def test_pinned_steps_continue_like_the_unpinned_ones(make, lens):
    net = make()
    prompt, cont = _tokens()
    steps, cap = cont.shape[1], TP + cont.shape[1] + 3

    def run(pin):
        net.rnnClearPreviousState()
        _step(net, prompt)
        if lens is not None:
            net.rnnTrimState(lens)
        if pin:
            net.rnnPinState(cap)
        return torch.cat([_step(net, cont[:, t:t + 1]) for t in range(steps)], 2)

    want, got = run(False), run(True)
    assert (got - want).abs().max() < 1e-9
    cached = net.layers[1] if make is _mln else net.layers_by_name["enc0"]
    emb = net.layers[0] if make is _mln else net.layers_by_name["emb"]
    assert cached._kv_len == cap - 1 and emb._seen == (cap - 1, len(LENS))   # the host's bound did not move
    assert cached._kv_short is emb._short is net._rnn_pin["short"]           # one array, not copies
    real = torch.tensor(lens if lens is not None else [TP] * len(LENS)) + steps
    assert torch.equal(cached._kv_short, (cap - 1 - real).to(torch.int32))
    assert net._rnn_pin["left"] == cap - TP - steps
    net.rnnClearPreviousState()
    assert not cached._kv_pinned and not emb._pinned and cached._kv is None


def test_the_stored_state_of_a_pinned_network_continues_on_a_fresh_one():
    net, other = _graph(), _new_mln()
    with torch.no_grad():
        other.flattenedParams.copy_(net.flattenedParams)
    prompt, cont = _tokens(3)
    cap = TP + 8
    net.rnnClearPreviousState()
    _step(net, prompt)
    net.rnnTrimState(LENS)
    net.rnnPinState(cap)
    for t in range(2):
        _step(net, cont[:, t:t + 1])
    states = net.rnnGetPreviousStates()
    real = torch.tensor(LENS) + 2
    for n in ("emb", "enc0", "enc1"):
        assert torch.equal(states[n]["short"], (cap - 1 - real).to(torch.int32))
        assert states[n]["short"] is not net._rnn_pin["short"]
    assert states["emb"]["pos"] == cap - 1 and states["enc0"]["kv"].shape == (4, cap - 1, 2 * E)
    want = [_step(net, cont[:, t:t + 1]) for t in (2, 3)]
    other.rnnClearPreviousState()
    for i, n in enumerate(("emb", "enc0", "enc1")):
        other.rnnSetPreviousState(i, states[n])
    assert other._rnn_pin is None                                # a ragged state of cap - 1 tokens seen, unpinned
    got = [_step(other, cont[:, t:t + 1]) for t in (2, 3)]
    assert other.layers[1]._kv_len == cap + 1
    for a, b in zip(got, want):
        assert (a - b).abs().max() < 1e-9
    net.rnnClearPreviousState()
    other.rnnClearPreviousState()


# ------------------------------------------------------------------------------------------------ refusals
def _pinned(net, cap, lens=None):
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    _step(net, prompt)
    if lens is not None:
        net.rnnTrimState(lens)
    net.rnnPinState(cap)
    return cont


def test_a_second_time_step_in_one_call_is_refused_and_changes_nothing():
    for net, who in ((_mln(), r"layer 0 \(BertEmbeddingLayer\)"), (_graph(), r"\(BertEmbeddingLayer\)")):
        cont = _pinned(net, TP + 5)
        before = net._rnn_pin["short"].clone()
        with pytest.raises(DL4JInvalidInputException, match=who + ".*exactly one time step"):
            _step(net, cont[:, :2])
        assert torch.equal(net._rnn_pin["short"], before) and net._rnn_pin["left"] == 5
        _step(net, cont[:, :1])
        assert net._rnn_pin["left"] == 4
        net.rnnClearPreviousState()


def test_a_cached_layer_refuses_a_second_time_step_itself():
    b = (NeuralNetConfiguration.Builder().seed(3).dataType(DataType.FLOAT).updater(NoOp()).list())
    b.layer(0, SelfAttentionLayer.Builder().nIn(V).nOut(8).nHeads(2).causal(True).activation(Activation.IDENTITY)
            .build())
    b.layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(8).nOut(V).build())
    net = MultiLayerNetwork(b.build())
    net.init(device=CPU)
    x = torch.randn(2, V, 5, generator=torch.Generator().manual_seed(0))
    net.rnnTimeStep(x)
    want = net.rnnTimeStep(x[:, :, :1])
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    net.rnnPinState(8)
    with pytest.raises(DL4JInvalidInputException, match=r"layer 0 \(SelfAttentionLayer\).*exactly one time step"):
        net.rnnTimeStep(x[:, :, :2])
    assert (net.rnnTimeStep(x[:, :, :1]) - want).abs().max() < 1e-6
    net.rnnClearPreviousState()


def test_capacity_exhausted_is_refused_before_anything_runs():
    net = _graph()
    cont = _pinned(net, TP + 2, LENS)                            # the longest row holds TP tokens: two steps
    _step(net, cont[:, :1])
    _step(net, cont[:, 1:2])
    before = {n: net.rnnGetPreviousState(n) for n in ("emb", "enc0", "enc1")}
    with pytest.raises(DL4JInvalidInputException, match=f"capacity of {TP + 2} positions is used up"):
        _step(net, cont[:, 2:3])
    for n, st in before.items():
        now = net.rnnGetPreviousState(n)
        assert torch.equal(now["short"], st["short"]) and ("kv" not in st or torch.equal(
            now["kv"].nan_to_num(), st["kv"].nan_to_num()))
    assert int(net._rnn_pin["short"].min()) == 0                 # the longest row reached the last cache row
    net.rnnClearPreviousState()


def test_capacity_out_of_range_is_refused_and_changes_nothing():
    net = _mln()
    prompt, cont = _tokens()
    net.rnnClearPreviousState()
    with pytest.raises(DL4JInvalidInputException, match="rnnPinState"):
        net.rnnPinState(20)                                      # nothing has gone through rnnTimeStep
    _step(net, prompt)
    with pytest.raises(DL4JInvalidInputException,
                       match=rf"layer 0 \(BertEmbeddingLayer\).*exceed maxPositions {MAXP}"):
        net.rnnPinState(MAXP + 1)
    with pytest.raises(DL4JInvalidInputException, match=r"rnnPinState.*capacity 9 leaves no room"):
        net.rnnPinState(TP)
    assert net._rnn_pin is None and not net.layers[1]._kv_pinned and net.layers[1]._kv_len == TP
    net.rnnPinState(MAXP)
    with pytest.raises(DL4JInvalidInputException, match="pinned already"):
        net.rnnPinState(MAXP)
    net.rnnClearPreviousState()


def _lstm_net():
    b = (NeuralNetConfiguration.Builder().seed(3).dataType(DataType.FLOAT).updater(NoOp()).list())
    b.layer(0, SelfAttentionLayer.Builder().nIn(V).nOut(8).nHeads(2).causal(True).activation(Activation.IDENTITY)
            .build())
    b.layer(1, LSTM.Builder().nIn(8).nOut(8).activation(Activation.TANH).build())
    b.layer(2, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(8).nOut(V).build())
    net = MultiLayerNetwork(b.build())
    net.init(device=CPU)
    return net


def test_a_network_with_an_lstm_is_refused_and_left_as_it_was():
    net = _lstm_net()
    x = torch.randn(2, V, 5, generator=torch.Generator().manual_seed(0))
    nxt = torch.randn(2, V, 1, generator=torch.Generator().manual_seed(1))
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    want = net.rnnTimeStep(nxt)
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    with pytest.raises(DL4JInvalidInputException, match=r"rnnPinState on layer 1 \(LSTM\)"):
        net.rnnPinState(12)
    assert net._rnn_pin is None and not net.layers[0]._kv_pinned and net.layers[0]._kv_len == 5
    assert torch.equal(net.rnnTimeStep(nxt), want)               # the refused call left no trace
    net.rnnClearPreviousState()
    with pytest.raises(DL4JInvalidInputException, match=r"rnnPinState on layer 1 \(LSTM\)"):
        net.generate(torch.tensor([[1, 2, 3], [4, 5, 0]]), inputEncoding="onehot", maxNewTokens=2, pinPositions=True)
    assert net.layers[0]._kv is None                             # refused before the prompt ran


def test_reorder_and_trim_are_refused_while_pinned():
    for net in (_mln(), _graph()):
        cont = _pinned(net, TP + 4)
        with pytest.raises(DL4JInvalidInputException, match="rnnReorderState.*pinned"):
            net.rnnReorderState(torch.tensor([1, 0, 2, 3], dtype=torch.int32))
        with pytest.raises(DL4JInvalidInputException, match="rnnTrimState.*pinned"):
            net.rnnTrimState(LENS)
        layer = net.layers[1] if hasattr(net, "layers") and not hasattr(net, "layers_by_name") else \
            net.layers_by_name["enc0"]
        with pytest.raises(DL4JInvalidInputException, match=r"rnnReorderState on layer .*TransformerEncoderLayer"):
            layer.rnnReorderState(torch.tensor([1, 0, 2, 3], dtype=torch.int32))
        _step(net, cont[:, :1])                                  # still in working order
        net.rnnClearPreviousState()
        _step(net, _tokens()[0])
        net.rnnTrimState(LENS)                                   # unpinned by the clear
        net.rnnClearPreviousState()


@pytest.mark.parametrize("field", ["useGraph", "pinPositions"])
def test_beam_search_is_refused_with_either_field(field):
    with pytest.raises(DL4JInvalidConfigException, match=field):
        GenerationConfig(numBeams=2, **{field: True}).validate()
    with pytest.raises(DL4JInvalidConfigException, match=field):
        _mln().generate(_tokens()[0], maxNewTokens=2, numBeams=3, **{field: True})
    assert GenerationConfig().useGraph is False and GenerationConfig().pinPositions is False


def test_use_graph_on_the_cpu_is_refused():
    net = _mln()
    net.rnnClearPreviousState()
    with pytest.raises(DL4JInvalidConfigException, match="useGraph"):
        net.generate(_tokens()[0], maxNewTokens=2, useGraph=True)
    assert net.layers[1]._kv is None


def test_the_commit_twin():
    from deeplearning4j_amd.ops import generation_native as GN
    short = torch.tensor([5, 0, 2, 1], dtype=torch.int32)
    step = torch.zeros(1, dtype=torch.int32)
    toks, lps = torch.full((2, 4), -1, dtype=torch.int64), torch.zeros(2, 4)
    for i in range(3):
        GN.step_commit(short, (step, torch.arange(4) + 10 * i, torch.full((4,), float(i)), toks, lps))
    assert short.tolist() == [2, 0, 0, 0] and int(step) == 2
    assert toks.tolist() == [[0, 1, 2, 3], [10, 11, 12, 13]] and lps.tolist() == [[0.0] * 4, [1.0] * 4]
