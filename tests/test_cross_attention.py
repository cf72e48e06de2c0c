"""Cross attention on the CPU: the reference / explicit ops against fp64 autograd, fp64 gradient checks of
CrossAttentionLayer and TransformerDecoderLayer as two-input graph layers (memory gradient summed over two blocks),
the builder rules (no merge vertex, exactly two inputs, graph-only), JSON / YAML round-trips, and rnnTimeStep with a
``None`` source against ``output()``, its refusal without a stored memory and the stored state's round-trip."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.gradientcheck import checkGradients
from deeplearning4j_amd.models import TransformerSeq2Seq
from deeplearning4j_amd.nn.conf.memory import MemoryUseMode
from deeplearning4j_amd.ops import transformer_native as TN


def _rand(*shape, seed=0, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------ ops
def test_reference_equals_self_attention_reference_on_one_sequence():
    B, T, H, D = 2, 7, 3, 4
    E = H * D
    qkv = _rand(B, T, 3 * E)
    mask = torch.ones(B, T, dtype=torch.float64)
    mask[1, 4:] = 0
    q, kv = qkv[:, :, :E].contiguous(), qkv[:, :, E:].contiguous()
    for m in (None, mask):
        ref = TN.attention_reference(qkv, H, m)
        got = TN.cross_attention_reference(q, kv, H, m)
        assert got.dtype == torch.float64 and (got - ref).abs().max().item() < 1e-12


def _ragged_mask(B, Tk, dead_row=None):
    m = torch.ones(B, Tk, dtype=torch.float64)
    m[0, Tk - 2:] = 0
    m[1, 1:] = 0                                  # one key only
    if dead_row is not None:
        m[dead_row] = 0
    return m


@pytest.mark.parametrize("masked", ["none", "ragged", "dead_row"])
def test_explicit_forward_backward_match_autograd_of_the_reference(masked):
    B, Tq, Tk, H, D = 3, 5, 9, 2, 4
    E = H * D
    q = _rand(B, Tq, E, seed=1).requires_grad_(True)
    kv = _rand(B, Tk, 2 * E, seed=2).requires_grad_(True)
    dout = _rand(B, Tq, E, seed=3)
    km = None if masked == "none" else _ragged_mask(B, Tk, 2 if masked == "dead_row" else None)
    ref = TN.cross_attention_reference(q, kv, H, km)
    rq, rkv = torch.autograd.grad(ref, (q, kv), dout)
    out, ctx = TN.cross_attention_fwd_explicit(q.detach(), kv.detach(), H, km)
    dq, dkv = TN.cross_attention_bwd_explicit(ctx, dout, torch.float64)
    assert dq.shape == (B, Tq, E) and dkv.shape == (B, Tk, 2 * E)
    for name, a, b in (("out", out, ref.detach()), ("dq", dq, rq), ("dkv", dkv, rkv)):
        assert torch.isfinite(a).all(), name
        assert (a - b).abs().max().item() < 1e-9, name
    if masked == "dead_row":                      # every key masked: zero output, zero gradients, no NaN
        assert out[2].abs().max() == 0 and dq[2].abs().max() == 0 and dkv[2].abs().max() == 0
        assert torch.isfinite(rq).all() and torch.isfinite(rkv).all()


# ------------------------------------------------------------------------------------------------ graphs
E, H, F, TQ, TK, MB, NM, V = 8, 2, 12, 4, 6, 3, 5, 7


def _builder(dt=DataType.DOUBLE):
    return (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
            .weightInit(NormalDistribution(0.0, 0.5)))


def _rnn_out(nIn=E, nOut=3):
    return RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(nIn).nOut(nOut).build()


def _cross_graph():
    g = _builder().graphBuilder()
    g.addInputs("x", "mem")
    g.addLayer("cross", CrossAttentionLayer.Builder().nIn(E).nInMemory(NM).nOut(E).nHeads(H)
               .activation(Activation.TANH).build(), "x", "mem")
    g.addLayer("out", _rnn_out(), "cross")
    g.setOutputs("out")
    return g


def _dec(nInMemory=E):
    return TransformerDecoderLayer.Builder().nIn(E).nInMemory(nInMemory).nOut(E).nHeads(H).ffnSize(F).build()


def _decoder_graph():
    """Two decoder blocks whose memory is a DenseLayer projection of the second input: the memory's gradient is
    summed over both blocks and flows on into the projection's weights."""
    g = _builder().graphBuilder()
    g.addInputs("x", "src")
    g.addLayer("proj", DenseLayer.Builder().nIn(NM).nOut(E).activation(Activation.TANH).build(), "src")
    g.addLayer("dec0", _dec(), "x", "proj")
    g.addLayer("dec1", _dec(), "dec0", "proj")
    g.addLayer("out", _rnn_out(), "dec1")
    g.setOutputs("out")
    g.setInputTypes(InputType.recurrent(E, TQ), InputType.recurrent(NM, TK))
    return g


def _net(g):
    net = ComputationGraph(g.build())
    net.init(device="cpu")
    return net


def _labels(T=TQ, n=3, seed=5):
    idx = torch.randint(0, n, (MB, T), generator=torch.Generator().manual_seed(seed))
    return torch.nn.functional.one_hot(idx, n).permute(0, 2, 1).to(torch.float64)


def _masks():
    qm = torch.ones(MB, TQ, dtype=torch.float64)
    qm[1, 3:] = 0
    km = torch.ones(MB, TK, dtype=torch.float64)
    km[0, 4:] = 0
    km[2, 1:] = 0
    return qm, km


def test_cross_attention_layer_gradients_two_inputs_of_different_lengths_both_masked():
    net = _net(_cross_graph())
    x, mem = _rand(MB, E, TQ, seed=1), _rand(MB, NM, TK, seed=2)
    qm, km = _masks()
    assert checkGradients(net, input=[x, mem], labels=[_labels()], inputMask=[qm, km], labelMask=[qm],
                          print_results=True)
    # masked query rows give zeros (before the activation: tanh(0) = 0); masked keys do not influence the output
    y = net.feedForward([x, mem], False, [qm, km])["cross"]
    assert y[1, :, 3:].abs().max() == 0
    mem2 = mem.clone()
    mem2[0, :, 4:] += 3.0
    y2 = net.feedForward([x, mem2], False, [qm, km])["cross"]
    assert (y - y2).abs().max().item() < 1e-12


def test_decoder_block_gradients_memory_summed_over_two_blocks():
    net = _net(_decoder_graph())
    x, src = _rand(MB, E, TQ, seed=1), _rand(MB, NM, TK, seed=2)
    _, km = _masks()
    assert checkGradients(net, input=[x, src], labels=[_labels()], inputMask=[None, km], print_results=True,
                          subset=600)
    # the projection's weights see both blocks: their gradient is not that of the last block alone
    net.computeGradientAndScore([x, src], [_labels()], [None, km])
    assert net.getLayer("proj").grads["W"].abs().max() > 0


def test_decoder_block_dropout_trains_on_the_cpu():
    g = _builder().graphBuilder()
    g.addInputs("x", "mem")
    g.addLayer("dec", TransformerDecoderLayer.Builder().nIn(E).nInMemory(E).nOut(E).nHeads(H).ffnSize(F)
               .hiddenDropout(0.25).attentionDropout(0.25).build(), "x", "mem")
    g.addLayer("out", _rnn_out(), "dec")
    g.setOutputs("out")
    net = _net(g)
    s = net.computeGradientAndScore([_rand(MB, E, TQ), _rand(MB, E, TK, seed=1)], [_labels()])
    assert torch.isfinite(torch.as_tensor(float(s))) and torch.isfinite(net.gradient().gradient()).all()


# ------------------------------------------------------------------------------------------------ builder
def test_no_merge_vertex_for_a_two_input_layer_and_types_inferred():
    conf = _decoder_graph().build()
    assert not any(n.endswith("-merge") for n in conf.vertices)
    assert conf.vertexInputs["dec0"] == ["x", "proj"] and conf.vertexInputs["dec1"] == ["dec0", "proj"]
    types = conf.getLayerActivationTypes()
    assert types["dec1"].size == E and types["dec1"].timeSeriesLength == TQ
    g = _builder().graphBuilder()
    g.addInputs("x", "mem")
    g.addLayer("cross", CrossAttentionLayer.Builder().nHeads(H).build(), "x", "mem")
    g.addLayer("out", _rnn_out(), "cross")
    g.setOutputs("out")
    g.setInputTypes(InputType.recurrent(E, TQ), InputType.recurrent(NM, TK))
    lc = g.build().vertices["cross"].layerConf
    assert (lc.nIn, lc.nInMemory, lc.nOut) == (E, NM, E)
    # an ordinary layer keeps its merge vertex
    g = _builder().graphBuilder()
    g.addInputs("a", "b")
    g.addLayer("d", DenseLayer.Builder().nIn(4).nOut(3).build(), "a", "b")
    g.addLayer("out", OutputLayer.Builder(LossFunction.MSE).nIn(3).nOut(2).build(), "d")
    g.setOutputs("out")
    assert "d-merge" in g.build().vertices


@pytest.mark.parametrize("inputs", [("x",), ("x", "mem", "x")])
def test_a_two_input_layer_needs_exactly_two_inputs(inputs):
    g = _builder().graphBuilder()
    g.addInputs("x", "mem")
    g.addLayer("cross", CrossAttentionLayer.Builder().nIn(E).nInMemory(E).nOut(E).nHeads(H).build(), *inputs)
    g.addLayer("out", _rnn_out(), "cross")
    g.setOutputs("out")
    g.allowDisconnected(True)
    with pytest.raises(DL4JInvalidConfigException, match="exactly two inputs"):
        g.build()


def test_multilayer_network_and_tbptt_refuse_a_two_input_layer():
    with pytest.raises(DL4JInvalidConfigException, match="ComputationGraph"):
        _builder().list().layer(0, _dec()).layer(1, _rnn_out()).build()
    g = _cross_graph()
    g.backpropType(BackpropType.TruncatedBPTT).tBPTTLength(2)
    with pytest.raises(DL4JInvalidConfigException, match="truncated BPTT"):
        g.build()


def test_json_and_yaml_round_trip():
    for g in (_cross_graph(), _decoder_graph()):
        conf = g.build()
        assert ComputationGraphConfiguration.fromJson(conf.toJson()) == conf
        assert ComputationGraphConfiguration.fromYaml(conf.toYaml()) == conf
    net = _net(_decoder_graph())
    assert "TransformerDecoderLayer" in net.summary()
    rep = net.conf.getMemoryReport(InputType.recurrent(E, TQ), InputType.recurrent(NM, TK))
    assert rep.getTotalMemoryBytes(2, MemoryUseMode.TRAINING) > rep.getTotalMemoryBytes(2, MemoryUseMode.INFERENCE) > 0


# ------------------------------------------------------------------------------------------------ rnnTimeStep
TS, TT = 5, 6


def _seq2seq(seed=12345):
    return TransformerSeq2Seq(numLabels=V, sourceVocabSize=9, seed=seed, inputShape=[TS, TT], hidden=E, layers=2,
                              heads=H, ffn=F, maxPositions=8, dataType=DataType.FLOAT).init(device="cpu")


def _tokens():
    gen = torch.Generator().manual_seed(0)
    src = torch.randint(0, 9, (MB, TS), generator=gen)
    tgt = torch.randint(0, V, (MB, TT), generator=gen)
    sm = torch.ones(MB, TS)
    sm[1, 3:] = 0
    return src, tgt, sm


@pytest.fixture(scope="module")
def seq2seq_and_ref():
    net = _seq2seq()
    src, tgt, sm = _tokens()
    ref = net.output(src, tgt, masks=[sm, None])[0].clone()
    return net, src, tgt, sm, ref


def test_time_step_with_none_source_equals_output_column_by_column(seq2seq_and_ref):
    net, src, tgt, sm, ref = seq2seq_and_ref
    assert ref.shape == (MB, V, TT)
    net.rnnClearPreviousState()
    y = net.rnnTimeStep(src, tgt[:, :1], masks=[sm, None])[0]
    assert y.shape == (MB, V, 1) and (y[:, :, 0] - ref[:, :, 0]).abs().max().item() < 1e-4
    for t in range(1, TT):
        y = net.rnnTimeStep(None, tgt[:, t:t + 1])[0]
        d = (y[:, :, 0] - ref[:, :, t]).abs().max().item()
        assert d < 1e-4, f"step {t}: rnnTimeStep differs from output() by {d}"
    # the source mask matters: the same run without it differs
    net.rnnClearPreviousState()
    y = net.rnnTimeStep(src, tgt[:, :1])[0]
    assert (y[1, :, 0] - ref[1, :, 0]).abs().max().item() > 1e-6
    # a first chunk of several target tokens
    net.rnnClearPreviousState()
    y = net.rnnTimeStep(src, tgt[:, :4], masks=[sm, None])[0]
    assert (y - ref[:, :, :4]).abs().max().item() < 1e-4


def test_time_step_without_a_stored_memory_raises(seq2seq_and_ref):
    net, src, tgt, sm, ref = seq2seq_and_ref
    net.rnnClearPreviousState()
    with pytest.raises(DL4JInvalidInputException, match="rnnClearPreviousState"):
        net.rnnTimeStep(None, tgt[:, :1])
    with pytest.raises(DL4JInvalidInputException):
        net.rnnTimeStep(None, None)
    net.rnnTimeStep(src, tgt[:, :1], masks=[sm, None])
    with pytest.raises(DL4JInvalidInputException, match="minibatch size"):
        net.rnnTimeStep(None, tgt[:2, 1:2])


def test_stored_state_round_trips_into_a_second_network(seq2seq_and_ref):
    net, src, tgt, sm, ref = seq2seq_and_ref
    net.rnnClearPreviousState()
    for t in range(3):
        net.rnnTimeStep(src if t == 0 else None, tgt[:, t:t + 1], masks=[sm, None] if t == 0 else None)
    st = net.rnnGetPreviousState("decoder_1")
    assert st["mem_kv"].shape == (MB, TS, 2 * E) and st["mem_mask"].shape == (MB, TS) and st["kv"].shape[1] == 3
    other = _seq2seq()
    other.setParams(net.params().clone())
    other.rnnSetPreviousStates(net.rnnGetPreviousStates())
    for t in range(3, TT):
        a = net.rnnTimeStep(None, tgt[:, t:t + 1])[0]
        b = other.rnnTimeStep(None, tgt[:, t:t + 1])[0]
        assert torch.equal(a, b)
        assert (a[:, :, 0] - ref[:, :, t]).abs().max().item() < 1e-4


def test_cross_attention_layer_time_step_keeps_its_memory():
    net = _net(_cross_graph())
    x, mem = _rand(MB, E, TQ, seed=1), _rand(MB, NM, TK, seed=2)
    _, km = _masks()
    ref = net.output(x, mem, masks=[None, km])[0]
    net.rnnClearPreviousState()
    ys = [net.rnnTimeStep(x[:, :, :1], mem, masks=[None, km])[0]]
    ys += [net.rnnTimeStep(x[:, :, t:t + 1], None)[0] for t in range(1, TQ)]
    assert (torch.cat(ys, 2) - ref).abs().max().item() < 1e-10


def test_seq2seq_fits():
    net = _seq2seq()
    src, tgt, sm = _tokens()
    lab = torch.nn.functional.one_hot(tgt, V).permute(0, 2, 1).float()
    s0 = float(net.computeGradientAndScore([src, tgt], [lab], [sm, None]))
    for _ in range(5):
        net.fit([src, tgt], [lab], featureMaskArrays=[sm, None])
    assert float(net.score()) < s0
