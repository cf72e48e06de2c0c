"""Llama-style transformer blocks on the CPU: ``normalization="rms"`` / ``normPlacement="pre"`` / ``ffnActivation="swiglu"``
on TransformerEncoderLayer and the RMSNormalization layer.

The two references against numbers worked out by hand; the configuration fields through the builder, JSON and YAML
and their refusals; parameter shapes, counts and the memory report; fp64 gradient checks of the three new block styles
and of RMSNormalization on both input ranks; the pre-norm block against a composition written here from plain torch
ops; chunked ``rnnTimeStep`` against ``output()`` (also with the fp8 cache and after ``rnnTrimState``); the zoo model
with its ``final_norm``, reproducible generation, and a save / load round trip."""
import io
import json
import math

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException
from deeplearning4j_amd.gradientcheck import checkGradients
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import transformer_native as TN
from deeplearning4j_amd.utils.model_serializer import ModelSerializer

V, E, H, HKV, F, T, MB = 11, 16, 4, 2, 24, 6, 2
D = E // H
EKV = HKV * D
LLAMA = ("rms", "pre", "swiglu")


def _builder(dt=DataType.DOUBLE, std=0.5):
    return (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
            .weightInit(NormalDistribution(0.0, std)))


def _enc(style=LLAMA, kv=HKV, cache=None, e=E, h=H, rotary=True, eps=1e-5, drop=0.0):
    norm, place, act = style
    return (TransformerEncoderLayer.Builder().nIn(e).nOut(e).nHeads(h).nKVHeads(kv).ffnSize(F).causal(True)
            .cacheDataType(cache).positionEncoding("rotary" if rotary else None).layerNormEps(eps)
            .hiddenDropout(drop).normalization(norm).normPlacement(place).ffnActivation(act).build())


def _lm(dt=DataType.DOUBLE, style=LLAMA, kv=HKV, cache=None, e=E, h=H, t=T, std=0.5, rotary=True):
    """tokens -> embeddings -> two causal blocks (-> final RMSNorm for a pre-norm stack) -> softmax"""
    g = _builder(dt, std).graphBuilder()
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(e).maxPositions(t + 2).inputLength(t)
               .positionEmbeddings(not rotary).build(), "tokens")
    g.addLayer("enc0", _enc(style, kv, cache, e, h, rotary), "emb")
    g.addLayer("enc1", _enc(style, kv, cache, e, h, rotary), "enc0")
    last = "enc1"
    if style[1] == "pre":
        g.addLayer("norm", RMSNormalization.Builder().nIn(e).nOut(e).build(), last)
        last = "norm"
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(e).nOut(V)
               .build(), last)
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device="cpu")
    return net


def _tokens(mb=MB, t=T, seed=0):
    return torch.randint(0, V, (mb, t), generator=torch.Generator().manual_seed(seed))


def _labels(t=T, seed=2, dt=torch.float64):
    y = torch.zeros(MB, V, t, dtype=dt)
    y.scatter_(1, torch.randint(0, V, (MB, 1, t), generator=torch.Generator().manual_seed(seed)), 1.0)
    return y


# ------------------------------------------------------------------------------------------------ the references
def test_rms_norm_reference_against_a_hand_written_example():
    """x = [3, 4, 0, 0]: mean(x^2) = 25/4, so with eps = 0 rstd = 2/5 and y = [1.2, 1.6, 0, 0] * gamma."""
    x = torch.tensor([[3.0, 4.0, 0.0, 0.0]], dtype=torch.float64)
    g = torch.tensor([1.0, 0.5, 2.0, 1.0], dtype=torch.float64)
    y, s, rstd = TN.rms_norm_reference(x, g, 0.0)
    assert s is x and abs(rstd.item() - 0.4) < 1e-15
    assert (y - torch.tensor([[1.2, 0.8, 0.0, 0.0]], dtype=torch.float64)).abs().max() < 1e-15
    # eps enters under the root: rstd = 1 / sqrt(25/4 + 2.75) = 1/3
    assert abs(TN.rms_norm_reference(x, g, 2.75)[2].item() - 1.0 / 3.0) < 1e-15
    # with a residual the sum is what is normalised and handed back
    r = torch.tensor([[-3.0, 0.0, 3.0, 0.0]], dtype=torch.float64)               # s = [0, 4, 3, 0]
    y2, s2, rstd2 = TN.rms_norm_reference(x, g, 0.0, r)
    assert s2.tolist() == [[0.0, 4.0, 3.0, 0.0]] and abs(rstd2.item() - 0.4) < 1e-15
    assert (y2 - torch.tensor([[0.0, 0.8, 2.4, 0.0]], dtype=torch.float64)).abs().max() < 1e-15
    # no mean is subtracted: a constant row maps to gamma, not to zero
    c = torch.full((1, 4), 7.0, dtype=torch.float64)
    assert (TN.rms_norm_reference(c, g, 0.0)[0] - g).abs().max() < 1e-15
    # the backward: finite differences of sum(y * w) in fp64
    w = torch.tensor([[0.3, -1.0, 0.7, 2.0]], dtype=torch.float64)
    xs = torch.tensor([[3.0, 4.0, -1.0, 0.5]], dtype=torch.float64)
    _, s3, rstd3 = TN.rms_norm_reference(xs, g, 1e-3)
    dx, dg = TN.rms_norm_backward_reference(w, s3, g, rstd3)
    for j in range(4):
        step = torch.zeros_like(xs)
        step[0, j] = 1e-6
        num = ((TN.rms_norm_reference(xs + step, g, 1e-3)[0] - TN.rms_norm_reference(xs - step, g, 1e-3)[0]) * w).sum()
        assert abs(num.item() / 2e-6 - dx[0, j].item()) < 1e-8
    assert (dg - (w * xs * rstd3)[0]).abs().max() < 1e-15
    # dres is added to the gradient
    dx2, _ = TN.rms_norm_backward_reference(w, s3, g, rstd3, dres=torch.ones_like(xs))
    assert (dx2 - dx - 1.0).abs().max() < 1e-15


def test_swiglu_reference_against_a_hand_written_example():
    """gu = [gate | up] with F = 2: silu(0) = 0, silu(ln 3) = ln 3 * 3/4 (sigmoid(ln 3) = 3/4)."""
    ln3 = math.log(3.0)
    gu = torch.tensor([[0.0, ln3, 5.0, -2.0]], dtype=torch.float64)
    out = TN.swiglu_reference(gu)
    assert out.shape == (1, 2)
    assert out[0, 0].item() == 0.0 and abs(out[0, 1].item() - ln3 * 0.75 * -2.0) < 1e-15
    # backward at g = 0: sig = 1/2, dg = df*u/2, du = 0; at g = ln 3: dg = df*u*(3/4)*(1 + ln3/4), du = df*ln3*3/4
    dgu = TN.swiglu_backward_reference(gu, torch.tensor([[2.0, 1.0]], dtype=torch.float64))
    want = torch.tensor([[2.0 * 5.0 * 0.5, -2.0 * 0.75 * (1.0 + ln3 * 0.25), 0.0, ln3 * 0.75]], dtype=torch.float64)
    assert (dgu - want).abs().max() < 1e-15
    # far out on both sides nothing overflows
    far = torch.tensor([[-800.0, 800.0, 3.0, 3.0]], dtype=torch.float64)
    assert TN.swiglu_reference(far).tolist() == [[-0.0, 2400.0]]
    assert torch.isfinite(TN.swiglu_backward_reference(far, torch.ones(1, 2, dtype=torch.float64))).all()


# ------------------------------------------------------------------------------------------------ configuration
def _plain_builder():
    return TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True)


def test_conf_fields_round_trip_and_the_defaults_leave_the_json_alone():
    plain = _plain_builder().build()
    assert (plain.normalization, plain.normPlacement, plain.ffnActivation) == ("layer", "post", "gelu")
    assert not plain.preNorm() and not plain.swiglu()
    text = plain.toJson()
    for name in ("normalization", "normPlacement", "ffnActivation"):
        assert name not in text
    assert TransformerEncoderLayer.fromJson(text) == plain
    llama = _plain_builder().normalization("rms").normPlacement("pre").ffnActivation("swiglu").build()
    d = json.loads(llama.toJson())
    assert (d["normalization"], d["normPlacement"], d["ffnActivation"]) == LLAMA
    back = TransformerEncoderLayer.fromJson(llama.toJson())
    assert back == llama and back != plain and back.preNorm() and back.swiglu()
    gated = _plain_builder().ffnActivation("swiglu").build()
    d = json.loads(gated.toJson())
    assert d["ffnActivation"] == "swiglu" and "normalization" not in d and "normPlacement" not in d
    assert TransformerEncoderLayer.fromJson(gated.toJson()) == gated
    rn = RMSNormalization.Builder().nIn(E).nOut(E).build()
    assert rn.eps == 1e-6 and RMSNormalization.fromJson(rn.toJson()) == rn
    assert RMSNormalization.Builder().nIn(E).nOut(E).eps(1e-5).build().eps == 1e-5


def test_network_conf_round_trips_through_json_and_yaml():
    net = _lm()
    text = net.conf.toJson()
    assert text.count('"normalization": "rms"') == 2 and text.count('"normPlacement": "pre"') == 2
    assert text.count('"ffnActivation": "swiglu"') == 2 and text.count('"RMSNormalization": {') == 1
    again = ComputationGraphConfiguration.fromJson(text)
    assert again.toJson() == text
    y = net.conf.toYaml()
    assert "normalization: rms" in y and "normPlacement: pre" in y and "ffnActivation: swiglu" in y
    assert ComputationGraphConfiguration.fromYaml(y).toJson() == text
    for t in (_lm(style=("layer", "post", "gelu")).conf.toJson(), _lm(style=("layer", "post", "gelu")).conf.toYaml()):
        assert "normalization" not in t and "normPlacement" not in t and "ffnActivation" not in t


@pytest.mark.parametrize("norm,place", [("layer", "pre"), ("rms", "post")])
def test_the_unsupported_combinations_are_refused_naming_the_layer(norm, place):
    b = _plain_builder().normalization(norm).normPlacement(place)
    with pytest.raises(DL4JInvalidConfigException, match=f"TransformerEncoderLayer.*{norm}.*{place}"):
        b.build()
    with pytest.raises(DL4JInvalidConfigException, match=f"TransformerEncoderLayer 'blk'.*{norm}.*{place}"):
        b.name("blk").build()
    with pytest.raises(DL4JInvalidConfigException, match=f"TransformerEncoderLayer 'blk'.*{norm}.*{place}"):
        b.ffnActivation("swiglu").build()


@pytest.mark.parametrize("field", ["normalization", "normPlacement", "ffnActivation"])
@pytest.mark.parametrize("bad", ["RMS", "Pre", "silu", "", None, 1, True])
def test_an_unknown_value_is_refused_naming_the_layer(field, bad):
    b = _plain_builder()
    with pytest.raises(DL4JInvalidConfigException, match=f"TransformerEncoderLayer.*{field}"):
        getattr(b, field)(bad).build()
    with pytest.raises(DL4JInvalidConfigException, match=f"TransformerEncoderLayer 'blk'.*{field}"):
        getattr(b.name("blk"), field)(bad).build()


def _shapes(conf):
    return {p.key: tuple(p.shape) for p in conf.param_specs()}


def test_parameter_shapes_counts_and_the_memory_report():
    Q = E + 2 * EKV
    common = {"Wqkv": (E, Q), "bqkv": (1, Q), "Wo": (E, E), "bo": (1, E), "ln1g": (1, E), "W2": (F, E), "b2": (1, E),
              "ln2g": (1, E)}
    attn = E * Q + Q + E * E + E
    cases = {
        ("layer", "post", "gelu"): (dict(common, ln1b=(1, E), ln2b=(1, E), W1=(E, F), b1=(1, F)),
                                    attn + 4 * E + E * F + F + F * E + E),
        ("layer", "post", "swiglu"): (dict(common, ln1b=(1, E), ln2b=(1, E), W1=(E, 2 * F), b1=(1, 2 * F)),
                                      attn + 4 * E + 2 * E * F + 2 * F + F * E + E),
        ("rms", "pre", "gelu"): (dict(common, W1=(E, F), b1=(1, F)), attn + 2 * E + E * F + F + F * E + E),
        ("rms", "pre", "swiglu"): (dict(common, W1=(E, 2 * F), b1=(1, 2 * F)),
                                   attn + 2 * E + 2 * E * F + 2 * F + F * E + E),
    }
    for style, (shapes, count) in cases.items():
        conf = _enc(style)
        assert _shapes(conf) == shapes, style
        assert conf.numParams() == count, style
        assert conf.is_bias("b1") and not conf.is_bias("ln1g") and not conf.is_bias("W1")
    assert RMSNormalization.Builder().nIn(E).nOut(E).build().numParams() == E
    assert _shapes(RMSNormalization.Builder().nIn(E).nOut(E).build()) == {"gamma": (1, E)}
    # the network holds what the configurations count, and the memory report agrees layer by layer
    net = _lm()
    rep = net.conf.getMemoryReport(InputType.recurrent(1, T))
    for name in ("enc0", "enc1"):
        assert rep.layerAndVertexReports[name].parameterSize == cases[LLAMA][1]
        assert sum(p.numel() for p in net.layers_by_name[name].params.values()) == cases[LLAMA][1]
        assert "ln1b" not in net.layers_by_name[name].params and "ln2b" not in net.layers_by_name[name].params
    assert rep.layerAndVertexReports["norm"].parameterSize == E
    assert sum(r.parameterSize for r in rep.layerAndVertexReports.values()) == net.numParams()


# ------------------------------------------------------------------------------------------------ gradient checks
@pytest.mark.parametrize("style,rotary,kv", [(LLAMA, True, HKV), (("rms", "pre", "gelu"), False, H),
                                              (("layer", "post", "swiglu"), False, H)],
                         ids=["rms-pre-swiglu", "rms-pre-gelu", "layer-post-swiglu"])
def test_block_gradients(style, rotary, kv):
    net = _lm(style=style, kv=kv, rotary=rotary)
    blk = net.layers_by_name["enc0"]
    assert tuple(blk.params["W1"].shape) == (E, 2 * F if style[2] == "swiglu" else F)
    assert ("ln1b" in blk.params) == (style[0] == "layer")
    assert checkGradients(net, input=[_tokens()], labels=[_labels()], print_results=True, subset=400)


def test_rms_normalization_gradients_on_both_input_ranks():
    gen = torch.Generator().manual_seed(1)
    # recurrent [mb, n, T]
    conf = (_builder().list()
            .layer(0, RMSNormalization.Builder().nIn(5).nOut(5).build())
            .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(5).nOut(3).build())
            .build())
    net = MultiLayerNetwork(conf)
    net.init(device="cpu")
    net.setParams(net.params() + 0.3 * torch.randn(net.numParams(), generator=gen, dtype=torch.float64))
    x = torch.randn(MB, 5, T, generator=gen, dtype=torch.float64)
    y = torch.zeros(MB, 3, T, dtype=torch.float64)
    y.scatter_(1, torch.randint(0, 3, (MB, 1, T), generator=gen), 1.0)
    assert checkGradients(net, input=x, labels=y, print_results=True)
    out = net.feedForward(x, False)[1]
    g = net.layers[0].params["gamma"].reshape(1, 5, 1)
    assert (out - x * torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-6) * g).abs().max() < 1e-12
    # feed-forward [mb, n]
    conf = (_builder().list()
            .layer(0, DenseLayer.Builder().nIn(4).nOut(5).activation(Activation.TANH).build())
            .layer(1, RMSNormalization.Builder().nIn(5).nOut(5).build())
            .layer(2, OutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(5).nOut(3).build())
            .build())
    net = MultiLayerNetwork(conf)
    net.init(device="cpu")
    net.setParams(net.params() + 0.3 * torch.randn(net.numParams(), generator=gen, dtype=torch.float64))
    x = torch.randn(5, 4, generator=gen, dtype=torch.float64)
    y = torch.zeros(5, 3, dtype=torch.float64)
    y.scatter_(1, torch.randint(0, 3, (5, 1), generator=gen), 1.0)
    assert checkGradients(net, input=x, labels=y, print_results=True)


# ------------------------------------------------------------------------------------------------ the block itself
def test_the_pre_norm_block_equals_a_composition_of_plain_torch_ops():
    """One block, fp32, written out from the formulas: rms = x * rsqrt(mean(x^2) + eps) * g, rotate_half RoPE, grouped
    causal softmax attention, silu(gate) * up."""
    eps = 1e-5
    conf = (_builder(DataType.FLOAT).list().layer(0, _enc(eps=eps))
            .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(3).build())
            .build())
    net = MultiLayerNetwork(conf)
    net.init(device="cpu")
    gen = torch.Generator().manual_seed(4)
    net.setParams(net.params() + 0.2 * torch.randn(net.numParams(), generator=gen))
    x = torch.randn(MB, E, T, generator=gen)
    got = net.feedForward(x, False)[1]
    P = net.layers[0].params

    def rms(v, g):
        return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * g.reshape(-1)

    def rope(v):                                                    # v [MB, T, heads, D]
        inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
        ang = (torch.arange(T, dtype=torch.float32)[:, None] * inv.float()[None, :]).double()
        cs, sn = torch.cos(ang).float()[None, :, None, :], torch.sin(ang).float()[None, :, None, :]
        a, b = v[..., :D // 2], v[..., D // 2:]
        return torch.cat([a * cs - b * sn, b * cs + a * sn], -1)

    xt = x.permute(0, 2, 1)                                          # [MB, T, E]
    qkv = rms(xt, P["ln1g"]) @ P["Wqkv"] + P["bqkv"]
    q = rope(qkv[..., :E].reshape(MB, T, H, D))
    k = rope(qkv[..., E:E + EKV].reshape(MB, T, HKV, D)).repeat_interleave(H // HKV, dim=2)
    v = qkv[..., E + EKV:].reshape(MB, T, HKV, D).repeat_interleave(H // HKV, dim=2)
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D)
    sc = sc.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
    ctx = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), v).reshape(MB, T, E)
    h = xt + ctx @ P["Wo"] + P["bo"]
    z = rms(h, P["ln2g"]) @ P["W1"] + P["b1"]
    want = h + (torch.nn.functional.silu(z[..., :F]) * z[..., F:]) @ P["W2"] + P["b2"]
    assert (got - want.permute(0, 2, 1)).abs().max() < 1e-5
    # and training with hidden dropout runs, drops something and leaves inference alone
    drop = MultiLayerNetwork((_builder(DataType.FLOAT).list().layer(0, _enc(eps=eps, drop=0.5))
                              .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX)
                                     .nIn(E).nOut(3).build()).build()))
    drop.init(device="cpu")
    drop.setParams(net.params().clone())
    assert torch.equal(drop.feedForward(x, False)[1], got)
    assert (drop.feedForward(x, True)[1] - got).abs().max() > 1e-3


# ------------------------------------------------------------------------------------------------ cached decoding
def _stream(net, x, chunks):
    outs, t = [], 0
    for n in chunks:
        outs.append(net.rnnTimeStep(x[:, t:t + n])[0])
        t += n
    assert t == x.shape[1]
    return torch.cat(outs, 2)


CHUNKS = (5, 1, 1, 3)


@pytest.mark.parametrize("style", [LLAMA, ("rms", "pre", "gelu"), ("layer", "post", "swiglu")],
                         ids=["rms-pre-swiglu", "rms-pre-gelu", "layer-post-swiglu"])
def test_chunked_time_step_equals_output(style):
    net = _lm(style=style, t=10)
    x = _tokens(t=10)
    ref = net.output(x)[0]
    net.rnnClearPreviousState()
    assert (_stream(net, x, CHUNKS) - ref).abs().max() < 1e-10
    assert (net.output(x.flip(1))[0].flip(2) - ref).abs().max() > 1e-3          # the order matters
    assert net.rnnGetPreviousState("enc0")["kv"].shape == (MB, 10, 2 * EKV)
    # one step at a time as [mb, 1] tokens
    net.rnnClearPreviousState()
    assert (_stream(net, x, (1,) * 10) - ref).abs().max() < 1e-10


def test_chunked_time_step_after_trim_equals_every_row_alone():
    net = _lm(t=10)
    x = _tokens(t=10, seed=3)
    lengths = [5, 3]
    rows = []
    for b, n in enumerate(lengths):                        # row b alone: its n prompt tokens, then the 5 that follow
        seq = torch.cat([x[b:b + 1, :n], x[b:b + 1, 5:]], 1)
        rows.append(net.output(seq)[0])
    net.rnnClearPreviousState()
    first = net.rnnTimeStep(x[:, :5])[0]
    net.rnnTrimState(lengths)
    rest = _stream(net, x[:, 5:], (1, 1, 3))
    for b, n in enumerate(lengths):
        assert (first[b, :, :n] - rows[b][0, :, :n]).abs().max() < 1e-10
        assert (rest[b] - rows[b][0, :, n:]).abs().max() < 1e-10


def test_chunked_time_step_with_the_fp8_cache():
    """The bound and the model (N(0, 0.05) weights, fp32) are those of the fp8 cache's own tests
    (tests/test_kv_cache_fp8.py, tests/test_rope.py): quantised, and no further off than 4 significant bits allow."""
    e, h, kv = 64, 4, 2
    net = _lm(DataType.FLOAT, LLAMA, kv, "fp8", e, h, t=10, std=0.05)
    twin = _lm(DataType.FLOAT, LLAMA, kv, None, e, h, t=10, std=0.05)
    twin.setParams(net.params().clone())
    x = _tokens(t=10, seed=5)
    ref = twin.output(x)[0]
    net.rnnClearPreviousState()
    got = _stream(net, x, CHUNKS)
    rel = ((got - ref).norm() / ref.norm()).item()
    assert 0 < rel < 5e-2, rel
    st = net.rnnGetPreviousState("enc1")
    assert st["kvFormat"] == "fp8" and st["kv"].shape == (MB, 10, TN.kv_fp8_row_bytes(h, e // h, kv))


# ------------------------------------------------------------------------------------------------ zoo, save / load
def _zoo(**kw):
    return TextGenerationTransformer(numLabels=V, inputShape=[T], hidden=E, layers=2, heads=H, ffn=F, nKVHeads=HKV,
                                     positionEncoding="rotary", **kw)


def test_the_zoo_model_builds_with_a_final_norm_and_generates_reproducibly():
    net = _zoo(normalization="rms", normPlacement="pre", ffnActivation="swiglu").init(device="cpu")
    assert list(net.layers_by_name) == ["embeddings", "decoder_0", "decoder_1", "final_norm", "output"]
    assert type(net.layers_by_name["final_norm"].conf).__name__ == "RMSNormalization"
    for i in range(2):
        c = net.layers_by_name[f"decoder_{i}"].conf
        assert c.preNorm() and c.swiglu() and c.normalization == "rms"
    assert "final_norm" not in _zoo().init(device="cpu").layers_by_name
    assert "normPlacement" not in _zoo().conf().toJson()
    # one training step moves every parameter block of a decoder block and the final norm
    p0 = net.params().clone()
    net.fit([_tokens()], [_labels(dt=torch.float32)])
    assert torch.isfinite(net.params()).all()
    for name in ("decoder_0", "final_norm"):
        for key, p in net.layers_by_name[name].params.items():
            assert p.abs().sum() > 0 and torch.isfinite(p).all(), (name, key)
    assert not torch.equal(p0, net.params())
    prompt = _tokens(t=4, seed=9)
    greedy = net.generate(prompt, maxNewTokens=12)
    assert greedy.tokens.shape == (MB, 12) and torch.equal(net.generate(prompt, maxNewTokens=12).tokens, greedy.tokens)
    pinned = net.generate(prompt, maxNewTokens=12, pinPositions=True)
    assert torch.equal(pinned.tokens, greedy.tokens)
    a = net.generate(prompt, maxNewTokens=12, doSample=True, temperature=1.3, seed=11)
    b = net.generate(prompt, maxNewTokens=12, doSample=True, temperature=1.3, seed=11)
    c = net.generate(prompt, maxNewTokens=12, doSample=True, temperature=1.3, seed=12)
    assert torch.equal(a.tokens, b.tokens) and not torch.equal(a.tokens, c.tokens)
    # the hand loop on rnnTimeStep gives the same greedy tokens
    net.rnnClearPreviousState()
    p = net.rnnTimeStep(prompt)[0][:, :, -1]
    for t in range(12):
        tok = p.argmax(1)
        assert torch.equal(tok, greedy.tokens[:, t])
        p = net.rnnTimeStep(tok.reshape(MB, 1))[0][:, :, -1]


def test_model_save_and_load_round_trips_the_new_parameters():
    net = _lm(DataType.FLOAT)
    gen = torch.Generator().manual_seed(6)
    net.setParams(net.params() + 0.1 * torch.randn(net.numParams(), generator=gen))
    buf = io.BytesIO()
    ModelSerializer.writeModel(net, buf, True)
    buf.seek(0)
    back = ModelSerializer.restoreComputationGraph(buf, True)
    assert back.conf.toJson() == net.conf.toJson()
    assert torch.equal(back.params(), net.params())
    for name in ("enc0", "norm"):
        for key, p in net.layers_by_name[name].params.items():
            assert torch.equal(back.layers_by_name[name].params[key], p), (name, key)
    x = _tokens()
    assert torch.equal(back.output(x)[0], net.output(x)[0])
