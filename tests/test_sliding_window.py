"""Sliding-window attention (``attentionWindow``) on the CPU: the references against a brute-force masked softmax
written here (fp64), the explicit forward / backward pair against ``torch.autograd`` on that formula, the
configuration field (refusals, JSON / YAML), ``TextGenerationTransformer(attentionWindow=...)`` and cached decoding
against ``output()`` on a model whose window is shorter than the sequence.

Query p sees keys k with p - W < k <= p: W keys, itself included (Mistral's ``sliding_window``)."""
import json
import math

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import transformer_native as TN

B, H, D, T = 2, 4, 8, 9
WINDOWS = [1, 3, T, T + 5]


def _case(Hkv, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, generator=g, dtype=torch.float64)
    dout = torch.randn(B, T, H * D, generator=g, dtype=torch.float64)
    mask = torch.ones(B, T)
    mask[1, 6:] = 0
    return qkv, dout, mask


def _brute(qkv, Hkv, W, mask=None):
    """softmax over the visible keys, one (b, h, q) at a time: key k is visible to query q when q - W < k <= q and
    the key-padding mask keeps it; a query with no visible key gives zeros."""
    G = H // Hkv
    E, Ekv = H * D, Hkv * D
    out = []
    for b in range(B):
        rows = []
        for q in range(T):
            heads = []
            for h in range(H):
                j = h // G
                qv = qkv[b, q, h * D:(h + 1) * D]
                ks = [k for k in range(T) if q - W < k <= q and (mask is None or mask[b, k] != 0)]
                if not ks:
                    heads.append(torch.zeros(D, dtype=qkv.dtype))
                    continue
                kk = torch.stack([qkv[b, k, E + j * D:E + (j + 1) * D] for k in ks])
                vv = torch.stack([qkv[b, k, E + Ekv + j * D:E + Ekv + (j + 1) * D] for k in ks])
                p = torch.softmax((kk @ qv) / math.sqrt(D), 0)
                heads.append(p @ vv)
            rows.append(torch.cat(heads))
        out.append(torch.stack(rows))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("Hkv", [4, 2, 1])
@pytest.mark.parametrize("W", WINDOWS)
def test_reference_equals_a_brute_force_masked_softmax(W, Hkv, masked):
    qkv, _, mask = _case(Hkv)
    m = mask if masked else None
    want = _brute(qkv, Hkv, W, m)
    got = TN.attention_reference(qkv, H, m, True, Hkv=Hkv, window=W)
    assert got.dtype == torch.float64 and (got - want).abs().max() < 1e-12
    out, _ = TN.attention_fwd_explicit(qkv, H, m, True, Hkv=Hkv, window=W)
    assert (out - want).abs().max() < 1e-12
    if W >= T:                                                 # the window sees the whole prefix: the call without it
        assert torch.equal(got, TN.attention_reference(qkv, H, m, True, Hkv=Hkv))
    else:
        assert (got - TN.attention_reference(qkv, H, m, True, Hkv=Hkv)).abs().max() > 1e-3


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("W", WINDOWS)
def test_explicit_backward_agrees_with_autograd_on_the_brute_force_formula(W, Hkv):
    qkv, dout, mask = _case(Hkv, seed=1)
    for m in (None, mask):
        leaf = qkv.clone().requires_grad_(True)
        (_brute(leaf, Hkv, W, m) * dout).sum().backward()
        out, ctx = TN.attention_fwd_explicit(qkv, H, m, True, Hkv=Hkv, window=W)
        got = TN.attention_bwd_explicit(ctx, dout, torch.float64)
        assert got.shape == qkv.shape and (got - leaf.grad).abs().max() < 1e-11


@pytest.mark.parametrize("W", [1, 3, 8, 40])
def test_decode_reference_is_the_tail_of_the_windowed_reference(W):
    Hkv, pos, Tn = 2, 5, 4
    qkv, _, _ = _case(Hkv, seed=2)
    E, Ekv = H * D, Hkv * D
    full = TN.attention_reference(qkv, H, None, True, Hkv=Hkv, window=W)
    got = TN.attention_decode_reference(qkv[:, pos:, :E], qkv[:, :, E:E + Ekv], qkv[:, :, E + Ekv:], H, pos, Hkv=Hkv,
                                        window=W)
    assert (got - full[:, pos:pos + Tn]).abs().max() < 1e-12
    # ragged: row 1 stands two positions earlier and sees two keys fewer at the far end of its window
    short = torch.tensor([0, 2], dtype=torch.int32)
    got = TN.attention_decode_reference(qkv[:, pos:, :E], qkv[:, :, E:E + Ekv], qkv[:, :, E + Ekv:], H, pos,
                                        short=short, Hkv=Hkv, window=W)
    alone = TN.attention_decode_reference(qkv[1:, pos:, :E], qkv[1:, :pos - 2 + Tn, E:E + Ekv],
                                          qkv[1:, :pos - 2 + Tn, E + Ekv:], H, pos - 2, Hkv=Hkv, window=W)
    assert (got[1] - alone[0]).abs().max() < 1e-12


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3"])
def test_the_ops_refuse_a_bad_window(bad):
    qkv, _, _ = _case(4)
    with pytest.raises(ValueError, match="window"):
        TN.attention_reference(qkv, H, None, True, window=bad)
    with pytest.raises(ValueError, match="window"):
        TN.attention_fwd_explicit(qkv, H, None, True, window=bad)
    with pytest.raises(ValueError, match="causal"):
        TN.attention_reference(qkv, H, None, False, window=3)


# ------------------------------------------------------------------------------------------------ configuration
E, F, V, MB = 16, 24, 11, 3


def _layer_builders(causal=True):
    return (SelfAttentionLayer.Builder().nIn(E).nOut(E).nHeads(H).causal(causal),
            TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(causal))


def test_a_window_on_a_bidirectional_layer_is_refused_naming_the_layer():
    for b, cls in zip(_layer_builders(False), ("SelfAttentionLayer", "TransformerEncoderLayer")):
        b.build()
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls}.*attentionWindow.*causal"):
            b.attentionWindow(4).build()
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls} 'blk'.*attentionWindow.*causal"):
            b.name("blk").attentionWindow(4).build()


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "4"])
def test_a_window_that_is_not_a_positive_integer_is_refused_naming_the_layer(bad):
    for b, cls in zip(_layer_builders(), ("SelfAttentionLayer", "TransformerEncoderLayer")):
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls}.*attentionWindow"):
            b.attentionWindow(bad).build()
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls} 'blk'.*attentionWindow"):
            b.name("blk").attentionWindow(bad).build()


def test_the_decoder_family_does_not_take_the_field():
    for cls in (CrossAttentionLayer, TransformerDecoderLayer):
        with pytest.raises((AttributeError, TypeError, DL4JInvalidConfigException), match=cls.__name__):
            cls.Builder().attentionWindow(4)
        with pytest.raises((AttributeError, TypeError, DL4JInvalidConfigException), match=cls.__name__):
            cls(nIn=E, nInMemory=E, nOut=E, nHeads=H, attentionWindow=4)
        assert "attentionWindow" not in cls.Builder().nIn(E).nInMemory(E).nOut(E).nHeads(H).build().toJson()


def test_layer_json_keeps_the_field_and_omits_it_at_none():
    for b in _layer_builders():
        plain = b.build()
        assert plain.attentionWindow is None and "attentionWindow" not in plain.toJson()
        win = b.attentionWindow(5).build()
        text = win.toJson()
        assert json.loads(text)["attentionWindow"] == 5
        back = type(win).fromJson(text)
        assert back == win and back != plain and back.attentionWindow == 5
        b.attentionWindow(None)


KW = dict(numLabels=V, hidden=E, layers=2, heads=H, ffn=F, inputShape=[12], nKVHeads=2, positionEncoding="rotary",
          normalization="rms", normPlacement="pre", ffnActivation="swiglu", seed=3)


def _lm(window, dt=DataType.FLOAT, **kw):
    return TextGenerationTransformer(attentionWindow=window, dataType=dt, **dict(KW, **kw)).init(device="cpu")


def _tokens(t=12, seed=0):
    return torch.randint(0, V, (MB, t), generator=torch.Generator().manual_seed(seed))


def test_network_conf_round_trips_through_json_and_yaml():
    net = _lm([5, None])
    text = net.conf.toJson()
    assert text.count('"attentionWindow": 5') == 1 and text.count("attentionWindow") == 1
    again = ComputationGraphConfiguration.fromJson(text)
    assert again.toJson() == text
    y = net.conf.toYaml()
    assert y.count("attentionWindow: 5") == 1
    assert ComputationGraphConfiguration.fromYaml(y).toJson() == text
    for t in (_lm(None).conf.toJson(), _lm(None).conf.toYaml()):
        assert "attentionWindow" not in t


def test_the_model_takes_an_int_or_one_entry_per_block():
    every = _lm(4)
    assert [every.layers_by_name[f"decoder_{i}"].conf.attentionWindow for i in range(2)] == [4, 4]
    mixed = _lm([None, 7])
    assert [mixed.layers_by_name[f"decoder_{i}"].conf.attentionWindow for i in range(2)] == [None, 7]
    assert _lm((3, 4)).layers_by_name["decoder_1"].conf.attentionWindow == 4
    for bad in ([4], [4, 4, 4], []):
        with pytest.raises(DL4JInvalidConfigException, match="attentionWindow.*2 blocks"):
            _lm(bad)
    with pytest.raises(DL4JInvalidConfigException, match="TransformerEncoderLayer.*attentionWindow"):
        _lm([4, 0])


# ------------------------------------------------------------------------------------------------ cached decoding
def _stream(net, x, chunks):
    outs, t = [], 0
    for n in chunks:
        outs.append(net.rnnTimeStep(x[:, t:t + n])[0])
        t += n
    assert t == x.shape[1]
    return torch.cat(outs, 2)


@pytest.mark.parametrize("chunks", [(1,) * 12, (5, 1, 4, 2), (12,)], ids=["steps", "chunked", "whole"])
@pytest.mark.parametrize("window", [5, [3, None], [None, 1]], ids=["5", "3+full", "full+1"])
def test_time_step_equals_output_with_a_window_shorter_than_the_sequence(window, chunks):
    """fp32, two blocks. The bound is the one tests/test_kv_cache_fp8.py holds an fp32 ``rnnTimeStep`` to against
    the same forward computed in one piece (1e-5 on softmax outputs)."""
    net = _lm(window)
    x = _tokens()
    ref = net.output(x)[0]
    net.rnnClearPreviousState()
    got = _stream(net, x, chunks)
    assert (got - ref).abs().max() < 1e-5
    # the window is in the forward: the same parameters without it give another output
    full = _lm(None)
    full.setParams(net.params().clone())
    assert (full.output(x)[0] - ref).abs().max() > 1e-6
    # the cache keeps every row
    assert net.rnnGetPreviousState("decoder_0")["kv"].shape[1] == 12


def test_a_window_as_long_as_the_sequence_changes_nothing():
    x = _tokens()
    full = _lm(None)
    want = full.output(x)[0]
    for window in (12, 13, 1000, [12, None]):
        net = _lm(window)
        net.setParams(full.params().clone())
        assert torch.equal(net.output(x)[0], want), window
        net.rnnClearPreviousState()
        full.rnnClearPreviousState()
        assert torch.equal(_stream(net, x, (5, 1, 6)), _stream(full, x, (5, 1, 6))), window


def test_windowed_block_gradients():
    from deeplearning4j_amd.gradientcheck import checkGradients
    net = _lm([3, None], DataType.DOUBLE, inputShape=[6])
    x = _tokens(6)
    y = torch.zeros(MB, V, 6, dtype=torch.float64)
    y.scatter_(1, torch.randint(0, V, (MB, 1, 6), generator=torch.Generator().manual_seed(2)), 1.0)
    assert checkGradients(net, input=[x], labels=[y], print_results=False, subset=300)


def test_self_attention_layer_streams_with_a_window():
    """SelfAttentionLayer takes the field too: fp64, token by token against ``output()``, and against the brute-force
    formula's effect (the window changes the output)."""
    def net(window):
        conf = (NeuralNetConfiguration.Builder().seed(7).dataType(DataType.DOUBLE).updater(NoOp())
                .weightInit(NormalDistribution(0.0, 0.5)).list()
                .layer(0, SelfAttentionLayer.Builder().nIn(5).nOut(E).nHeads(H).nKVHeads(2).causal(True)
                       .positionEncoding("rotary").attentionWindow(window).build())
                .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(3)
                       .build()).build())
        n = MultiLayerNetwork(conf)
        n.init(device="cpu")
        return n
    win, full = net(3), net(None)
    full.setParams(win.params().clone())
    x = torch.randn(MB, 5, 8, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    ref = win.output(x)
    assert (full.output(x) - ref).abs().max() > 1e-4
    assert torch.equal(full.output(x)[:, :, :3], ref[:, :, :3])          # the first W queries see their whole prefix
    win.rnnClearPreviousState()
    got = torch.cat([win.rnnTimeStep(x[:, :, t:t + 1]) for t in range(8)], 2)
    assert (got - ref).abs().max() < 1e-10
