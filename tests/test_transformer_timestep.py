"""rnnTimeStep of the causal transformer layers on the CPU (fp64): feeding a sequence in pieces through the cached
key/value state must reproduce ``output()`` on the whole sequence, for ComputationGraph and MultiLayerNetwork, for
the encoder block and the plain SelfAttentionLayer; the stored state round-trips; a changed minibatch size and a
step past ``maxPositions`` raise; a bidirectional block keeps its behaviour; the zoo model trains and generates."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidInputException
from deeplearning4j_amd.models import TextGenerationTransformer

V, E, H, F, T, MB = 11, 16, 4, 24, 6, 3
TOL = 1e-10


def _builder():
    return (NeuralNetConfiguration.Builder().seed(7).dataType(DataType.DOUBLE).updater(NoOp())
            .weightInit(NormalDistribution(0.0, 0.5)))


def _emb(maxPositions=T + 2):
    return BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(maxPositions).inputLength(T).build()


def _enc(causal=True):
    return TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(causal).build()


def _out():
    return RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V).build()


def _graph(causal=True, maxPositions=T + 2):
    g = _builder().graphBuilder()
    g.addInputs("tokens")
    g.addLayer("emb", _emb(maxPositions), "tokens")
    g.addLayer("enc0", _enc(causal), "emb")
    g.addLayer("enc1", _enc(causal), "enc0")
    g.addLayer("out", _out(), "enc1")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device="cpu")
    return net


def _mln():
    conf = (_builder().list().layer(0, _emb()).layer(1, _enc()).layer(2, _enc()).layer(3, _out()).build())
    net = MultiLayerNetwork(conf)
    net.init(device="cpu")
    return net


def _tokens(mb=MB, seed=0):
    return torch.randint(0, V, (mb, T), generator=torch.Generator().manual_seed(seed))


def _full(net, x):
    y = net.output(x)
    return y[0] if isinstance(y, (list, tuple)) else y


def _step(net, x):
    y = net.rnnTimeStep(x)
    return y[0] if isinstance(y, (list, tuple)) else y


def _stream(net, x, chunks):
    """Outputs of feeding x [mb, T] (or [mb, n, T]) through rnnTimeStep in pieces of the given sizes, joined in time."""
    outs, t = [], 0
    for n in chunks:
        outs.append(_step(net, x[..., t:t + n]))
        t += n
    assert t == x.shape[-1]
    return torch.cat(outs, 2)


@pytest.fixture(scope="module", params=["graph", "mln"])
def net_and_ref(request):
    net = _graph() if request.param == "graph" else _mln()
    x = _tokens()
    return net, x, _full(net, x).clone()


def test_token_by_token_equals_whole_sequence(net_and_ref):
    net, x, ref = net_and_ref
    net.rnnClearPreviousState()
    for t in range(T):
        y = _step(net, x[:, t:t + 1])
        assert y.shape == (MB, V, 1)
        d = (y[:, :, 0] - ref[:, :, t]).abs().max().item()
        assert d <= TOL, f"step {t}: rnnTimeStep differs from output() by {d}"


def test_uneven_chunks_equal_whole_sequence(net_and_ref):
    net, x, ref = net_and_ref
    net.rnnClearPreviousState()
    y = _stream(net, x, (2, 1, 3))
    assert (y - ref).abs().max().item() <= TOL


def test_self_attention_layer_token_by_token():
    conf = (_builder().list()
            .layer(0, SelfAttentionLayer.Builder().nIn(E).nOut(E).nHeads(H).causal(True).build())
            .layer(1, _out()).build())
    net = MultiLayerNetwork(conf)
    net.init(device="cpu")
    x = torch.randn(MB, E, T, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    ref = _full(net, x)
    net.rnnClearPreviousState()
    for t in range(T):
        d = (_step(net, x[:, :, t:t + 1])[:, :, 0] - ref[:, :, t]).abs().max().item()
        assert d <= TOL, f"step {t}: rnnTimeStep differs from output() by {d}"
    net.rnnClearPreviousState()                      # a 2-d input is one step and returns 2-d
    y0 = _step(net, x[:, :, 0])
    assert y0.shape == (MB, V) and (y0 - ref[:, :, 0]).abs().max().item() <= TOL


def test_state_round_trip():
    net = _graph()
    x = _tokens()
    ref = _full(net, x)
    net.rnnClearPreviousState()
    for t in range(3):
        _step(net, x[:, t:t + 1])
    saved = net.rnnGetPreviousStates()
    kv = saved["enc0"]["kv"]
    assert kv.shape == (MB, 3, 2 * E)
    first = [_step(net, x[:, t:t + 1]).clone() for t in range(3, 6)]
    net.rnnClearPreviousState()
    net.rnnSetPreviousStates(saved)
    again = [_step(net, x[:, t:t + 1]) for t in range(3, 6)]
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    net.rnnClearPreviousState()
    assert net.rnnGetPreviousState("enc0") == {}
    assert (_step(net, x[:, 0:1])[:, :, 0] - ref[:, :, 0]).abs().max().item() <= TOL


def test_state_reaches_layers_of_multilayer_network():
    net = _mln()
    x = _tokens()
    net.rnnClearPreviousState()
    y0 = _step(net, x[:, 0:2]).clone()
    assert net.rnnGetPreviousState(1)["kv"].shape == (MB, 2, 2 * E)
    saved = [net.rnnGetPreviousState(i) for i in range(3)]
    y1 = _step(net, x[:, 2:3]).clone()
    net.rnnClearPreviousState()
    for i, st in enumerate(saved):
        net.rnnSetPreviousState(i, st)
    assert torch.equal(_step(net, x[:, 2:3]), y1)
    net.rnnClearPreviousState()
    assert torch.equal(_step(net, x[:, 0:2]), y0)


def test_changed_minibatch_raises():
    net = _graph()
    x = _tokens()
    net.rnnClearPreviousState()
    _step(net, x[:, 0:1])
    with pytest.raises(DL4JInvalidInputException):
        _step(net, x[:2, 1:2])
    enc = net.layers_by_name["enc0"]                 # the block itself checks too, not only the embedding before it
    with pytest.raises(DL4JInvalidInputException, match="minibatch size 2 differs from the stored state's 3"):
        enc.rnnTimeStep(torch.zeros(2, E, 1, dtype=torch.float64))
    net.rnnClearPreviousState()
    assert _step(net, x[:2, 0:1]).shape == (2, V, 1)


def test_step_past_max_positions_raises():
    net = _graph(maxPositions=T)
    x = _tokens()
    net.rnnClearPreviousState()
    _stream(net, x, (4, 2))
    with pytest.raises(DL4JInvalidInputException, match="maxPositions"):
        _step(net, x[:, 0:1])


def test_non_causal_block_is_unchanged():
    net = _graph(causal=False)
    x = _tokens()
    net.rnnClearPreviousState()
    chunk = x[:, 0:4]
    assert torch.equal(_step(net, chunk), _full(net, chunk))
    enc = net.layers_by_name["enc0"]
    h = torch.randn(MB, E, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert torch.equal(enc.rnnTimeStep(h), enc.activate(h, False))
    assert torch.equal(enc.rnnTimeStep(h), enc.activate(h, False))      # no state carried between calls


def test_zoo_text_generation_transformer():
    net = TextGenerationTransformer(numLabels=V, inputShape=[T], hidden=32, layers=2, heads=2, ffn=64,
                                    maxPositions=16, dataType=DataType.DOUBLE, learningRate=1e-2).init(device="cpu")
    x = _tokens(mb=4, seed=2)
    y = torch.nn.functional.one_hot(torch.roll(x, -1, 1), V).permute(0, 2, 1).to(torch.float64)
    for _ in range(3):
        net.fit([x], [y])
        s = net.score()
        assert s == s and abs(s) < 1e6, f"score {s}"
    ref = _full(net, x)
    net.rnnClearPreviousState()
    for t in range(T):
        d = (_step(net, x[:, t:t + 1])[:, :, 0] - ref[:, :, t]).abs().max().item()
        assert d <= TOL, f"step {t}: rnnTimeStep differs from output() by {d}"
