"""Rotary position embeddings (``positionEncoding="rotary"``) on the CPU: ``rope_reference`` against numbers worked
out by hand, the relative-position property, the inverse and the untouched V columns; the configuration fields in
JSON / YAML and their refusals; fp64 gradient checks of a rotary SelfAttentionLayer and a rotary causal
TransformerEncoderLayer with grouped heads; chunked ``rnnTimeStep`` against ``output()`` (16-bit and fp8 cache, also
after ``rnnTrimState``); an embedding layer without a position table and generation past ``maxPositions``."""
import json

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.gradientcheck import checkGradients
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import transformer_native as TN

V, E, H, HKV, F, T, MB = 11, 16, 4, 2, 24, 6, 2
D = E // H
EKV = HKV * D
THETA = 10000.0


def _builder(dt=DataType.DOUBLE, std=0.5):
    return (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
            .weightInit(NormalDistribution(0.0, std)))


def _enc(kv=HKV, cache=None, e=E, h=H, rotary=True, theta=THETA):
    return (TransformerEncoderLayer.Builder().nIn(e).nOut(e).nHeads(h).nKVHeads(kv).ffnSize(F).causal(True)
            .cacheDataType(cache).positionEncoding("rotary" if rotary else None).ropeTheta(theta).build())


def _lm(dt=DataType.DOUBLE, kv=HKV, cache=None, e=E, h=H, t=T, std=0.5, rotary=True):
    """tokens -> embeddings (no position table when rotary) -> two causal blocks -> softmax over the vocabulary"""
    g = _builder(dt, std).graphBuilder()
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(e).maxPositions(t + 2).inputLength(t)
               .positionEmbeddings(not rotary).build(), "tokens")
    g.addLayer("enc0", _enc(kv, cache, e, h, rotary), "emb")
    g.addLayer("enc1", _enc(kv, cache, e, h, rotary), "enc0")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(e).nOut(V)
               .build(), "enc1")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device="cpu")
    return net


def _tokens(mb=MB, t=T, seed=0):
    return torch.randint(0, V, (mb, t), generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_against_a_hand_written_example():
    """One head of size 4, theta = 16: inv_freq = [1, 1/4]. Token 0 at position 0 is left alone; token 1 at position 2
    is rotated by the angles [2, 0.5]: out[j] = x[j] cos - x[j+2] sin, out[j+2] = x[j+2] cos + x[j] sin."""
    assert TN.rope_inv_freq(4, 16.0, "cpu").tolist() == [1.0, 0.25]
    q, k, v = [1.0, 2.0, 3.0, 4.0], [0.5, -1.0, 2.0, 0.0], [9.0, 8.0, 7.0, 6.0]
    qkv = torch.tensor([[q + k + v, q + k + v]], dtype=torch.float64)
    got = TN.rope_reference(qkv, 1, torch.tensor([[0, 2]]), 16.0)
    assert torch.equal(got[0, 0], qkv[0, 0])
    # cos 2 = -0.4161468365471424, sin 2 = 0.9092974268256817, cos .5 = 0.8775825618903728, sin .5 = 0.479425538604203
    want = torch.tensor([-3.1440391170241874, -0.1625370306360665, -0.3391430828157456, 4.469181324769897,
                         -2.0266682719249346, -0.8775825618903728, -0.37764495968144395, -0.479425538604203,
                         9.0, 8.0, 7.0, 6.0], dtype=torch.float64)
    assert (got[0, 1] - want).abs().max() < 1e-14
    inv = TN.rope_reference(qkv, 1, torch.tensor([[0, 2]]), 16.0, inverse=True)
    # the inverse rotates the other way: the first pair of q
    assert abs(inv[0, 1, 0].item() - (1.0 * -0.4161468365471424 + 3.0 * 0.9092974268256817)) < 1e-14


@pytest.mark.parametrize("kv", [4, 2, 1])
def test_scores_depend_on_the_distance_only_and_the_inverse_undoes(kv):
    """theta = 256 with D = 8 gives inv_freq = 4^-j, exact in fp32, so the fp32 angle p * inv_freq is the exact one
    for every integer position here and the property holds to fp64 rounding."""
    d, theta, t = 8, 256.0, 9
    assert TN.rope_inv_freq(d, theta, "cpu").tolist() == [1.0, 0.25, 0.0625, 0.015625]
    gen = torch.Generator().manual_seed(kv)
    qkv = torch.randn(2, t, (H + 2 * kv) * d, generator=gen, dtype=torch.float64)
    pos = torch.arange(t).reshape(1, t) + torch.tensor([[0], [11]])

    def scores(p):
        q, k, _ = TN.gqa_split(TN.rope_reference(qkv, H, p, theta, Hkv=kv), H, kv)
        k = k.repeat_interleave(H // kv, dim=2)
        return torch.einsum("bmhd,bnhd->bhmn", q, k)

    assert (scores(pos) - scores(pos + 37)).abs().max() < 1e-9
    assert (scores(pos) - scores(pos * 0)).abs().max() > 1e-2               # and the rotation does something
    rot = TN.rope_reference(qkv, H, pos, theta, Hkv=kv)
    n = (H + kv) * d
    assert torch.equal(rot[..., n:], qkv[..., n:])                           # V bit-identical
    assert not torch.equal(rot[..., :n], qkv[..., :n])
    back = TN.rope_reference(rot, H, pos, theta, Hkv=kv, inverse=True)
    assert (back - qkv).abs().max() < 1e-12
    assert torch.equal(back[..., n:], qkv[..., n:])


def test_positions_follow_the_cache_rows():
    short = torch.tensor([0, 3, 99, -5], dtype=torch.int32)
    got = TN.rope_positions(4, 2, 7, short)
    assert got.tolist() == [[7, 8], [4, 5], [0, 1], [7, 8]]                  # the shortfall is clamped into [0, pos]
    assert TN.rope_positions(2, 3, 5).tolist() == [[5, 6, 7], [5, 6, 7]]
    assert TN.rope_inv_freq(64, 10000.0, "cpu") is TN.rope_inv_freq(64, 10000.0, torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ configuration
def _layer_builders():
    return [SelfAttentionLayer.Builder().nIn(E).nOut(E).nHeads(H).causal(True),
            TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True)]


def test_conf_fields_round_trip_and_the_defaults_leave_the_json_alone():
    for b in _layer_builders():
        plain = b.build()
        assert plain.positionEncoding is None and plain.ropeTheta == 10000.0 and not plain.rotary()
        text = plain.toJson()
        assert "positionEncoding" not in text and "ropeTheta" not in text
        assert type(plain).fromJson(text) == plain
        rot = b.positionEncoding("rotary").build()
        d = json.loads(rot.toJson())
        assert d["positionEncoding"] == "rotary" and "ropeTheta" not in d
        assert rot.rotary() and rot.numParams() == plain.numParams()
        rot2 = b.ropeTheta(500000).build()
        text2 = rot2.toJson()
        assert json.loads(text2)["ropeTheta"] == 500000.0
        back = type(rot2).fromJson(text2)
        assert back == rot2 and back != rot and back != plain and back.ropeTheta == 500000.0 and back.rotary()
        b.positionEncoding(None).ropeTheta(10000.0)


def test_network_conf_round_trips_through_json_and_yaml():
    net = _lm()
    text = net.conf.toJson()
    assert text.count('"positionEncoding": "rotary"') == 2 and text.count('"positionEmbeddings": false') == 1
    again = ComputationGraphConfiguration.fromJson(text)
    assert again.toJson() == text
    y = net.conf.toYaml()
    assert "positionEncoding: rotary" in y and "positionEmbeddings: false" in y
    assert ComputationGraphConfiguration.fromYaml(y).toJson() == text
    for t in (_lm(rotary=False).conf.toJson(), _lm(rotary=False).conf.toYaml()):
        assert "positionEncoding" not in t and "ropeTheta" not in t and "positionEmbeddings" not in t


@pytest.mark.parametrize("bad", ["rope", "Rotary", 1, True, ""])
def test_an_unknown_position_encoding_is_refused_naming_the_layer(bad):
    for b, cls in zip(_layer_builders(), ("SelfAttentionLayer", "TransformerEncoderLayer")):
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls}.*positionEncoding"):
            b.positionEncoding(bad).build()
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls} 'blk'.*positionEncoding"):
            b.name("blk").positionEncoding(bad).build()


@pytest.mark.parametrize("bad", [0, -1.0, float("inf"), float("nan"), "1e4", None, True])
def test_a_theta_that_is_not_finite_and_positive_is_refused_naming_the_layer(bad):
    for b, cls in zip(_layer_builders(), ("SelfAttentionLayer", "TransformerEncoderLayer")):
        with pytest.raises(DL4JInvalidConfigException, match=f"{cls} 'blk'.*ropeTheta"):
            b.name("blk").positionEncoding("rotary").ropeTheta(bad).build()


def test_an_odd_head_size_is_refused_with_rotary_only():
    att = SelfAttentionLayer.Builder().nIn(E).nOut(15).nHeads(3).name("att")
    enc = TransformerEncoderLayer.Builder().nIn(15).nOut(15).nHeads(3).ffnSize(F).name("enc")
    hs = SelfAttentionLayer.Builder().nIn(E).nOut(E).nHeads(H).headSize(7).name("hs")
    for b, who in ((att, "SelfAttentionLayer 'att'"), (enc, "TransformerEncoderLayer 'enc'"),
                   (hs, "SelfAttentionLayer 'hs'")):
        b.build()                                                           # fine without rotary
        with pytest.raises(DL4JInvalidConfigException, match=f"{who}.*even head size"):
            b.positionEncoding("rotary").build()
    # a block whose width comes from the input type is refused when the network configuration is built
    late = TransformerEncoderLayer.Builder().nHeads(3).ffnSize(F).name("late").positionEncoding("rotary").build()
    with pytest.raises(DL4JInvalidConfigException, match="TransformerEncoderLayer 'late'.*even head size"):
        (_builder().list().layer(0, late)
         .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nOut(3).build())
         .setInputType(InputType.recurrent(15, T)).build())


def test_the_decoder_family_has_no_such_setter():
    for cls in (TransformerDecoderLayer, CrossAttentionLayer):
        b = cls.Builder()
        for name in ("positionEncoding", "ropeTheta"):
            with pytest.raises((AttributeError, TypeError, DL4JInvalidConfigException)):
                getattr(b, name)("rotary")
        assert "positionEncoding" not in cls.Builder().nIn(E).nInMemory(E).nOut(E).nHeads(H).build().toJson()


# ------------------------------------------------------------------------------------------------ gradient checks
def test_rotary_self_attention_layer_gradients():
    conf = (_builder().list()
            .layer(0, SelfAttentionLayer.Builder().nIn(5).nOut(E).nHeads(H).causal(False).positionEncoding("rotary")
                   .activation(Activation.TANH).build())
            .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(3).build())
            .build())
    net = MultiLayerNetwork(conf)
    net.init(device="cpu")
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(MB, 5, T, generator=gen, dtype=torch.float64)
    y = torch.zeros(MB, 3, T, dtype=torch.float64)
    y.scatter_(1, torch.randint(0, 3, (MB, 1, T), generator=gen), 1.0)
    assert checkGradients(net, input=x, labels=y, print_results=True)
    # the rotation is in the forward: the same parameters without it give another output
    plain = MultiLayerNetwork((_builder().list()
                               .layer(0, SelfAttentionLayer.Builder().nIn(5).nOut(E).nHeads(H).causal(False)
                                      .activation(Activation.TANH).build())
                               .layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX)
                                      .nIn(E).nOut(3).build()).build()))
    plain.init(device="cpu")
    plain.setParams(net.params().clone())
    assert (plain.output(x) - net.output(x)).abs().max() > 1e-3


def test_rotary_causal_transformer_block_gradients_with_grouped_heads():
    net = _lm()
    blk = net.layers_by_name["enc0"]
    assert blk.conf.rotary() and blk.conf.nKVHeads == HKV
    assert tuple(blk.params["Wqkv"].shape) == (E, E + 2 * EKV)
    x = _tokens()
    y = torch.zeros(MB, V, T, dtype=torch.float64)
    y.scatter_(1, torch.randint(0, V, (MB, 1, T), generator=torch.Generator().manual_seed(2)), 1.0)
    assert checkGradients(net, input=[x], labels=[y], print_results=True, subset=400)


# ------------------------------------------------------------------------------------------------ cached decoding
def _stream(net, x, chunks):
    outs, t = [], 0
    for n in chunks:
        outs.append(net.rnnTimeStep(x[:, t:t + n])[0])
        t += n
    assert t == x.shape[1]
    return torch.cat(outs, 2)


CHUNKS = (5, 1, 1, 3)


def test_chunked_time_step_equals_output():
    net = _lm(t=10)
    x = _tokens(t=10)
    ref = net.output(x)[0]
    net.rnnClearPreviousState()
    assert (_stream(net, x, CHUNKS) - ref).abs().max() < 1e-10
    # without positions anywhere a causal model would still pass the check above: this one depends on the order
    assert (net.output(x.flip(1))[0].flip(2) - ref).abs().max() > 1e-3
    st = net.rnnGetPreviousState("enc0")
    assert st["kv"].shape == (MB, 10, 2 * EKV)
    # the cache holds ROTATED keys: row r of K is the projection's K rotated by r
    blk = net.layers_by_name["enc0"]
    h0 = net.feedForward([x], False)["emb"].permute(0, 2, 1).reshape(MB * 10, E)
    qkv = (h0 @ blk.params["Wqkv"] + blk.params["bqkv"]).reshape(MB, 10, -1)
    rot = TN.rope_reference(qkv, H, torch.arange(10), THETA, Hkv=HKV)
    assert (st["kv"] - rot[..., E:]).abs().max() < 1e-10
    assert (st["kv"][..., :EKV] - qkv[..., E:E + EKV]).abs().max() > 1e-3


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
    (tests/test_kv_cache_fp8.py, tests/test_gqa.py): quantised, and no further off than 4 significant bits allow."""
    e, h, kv = 64, 4, 2
    net = _lm(DataType.FLOAT, kv, "fp8", e, h, t=10, std=0.05)
    twin = _lm(DataType.FLOAT, kv, None, e, h, t=10, std=0.05)
    twin.setParams(net.params().clone())
    x = _tokens(t=10, seed=5)
    ref = twin.output(x)[0]
    net.rnnClearPreviousState()
    got = _stream(net, x, CHUNKS)
    rel = ((got - ref).norm() / ref.norm()).item()
    assert 0 < rel < 5e-2, rel
    st = net.rnnGetPreviousState("enc1")
    assert st["kvFormat"] == "fp8" and st["kv"].shape == (MB, 10, TN.kv_fp8_row_bytes(h, e // h, kv))


# ------------------------------------------------------------------------------------------------ no position table
def _zoo(rotary, maxPositions=16):
    return TextGenerationTransformer(numLabels=V, inputShape=[T], hidden=E, layers=2, heads=H, ffn=F, nKVHeads=HKV,
                                     maxPositions=maxPositions, positionEncoding="rotary" if rotary else None)


def test_an_embedding_without_positions_has_no_table():
    learned, rotary = _zoo(False).init(device="cpu"), _zoo(True).init(device="cpu")
    assert "Wpos" in learned.layers_by_name["embeddings"].params
    assert "Wpos" not in rotary.layers_by_name["embeddings"].params
    assert "Wpos" not in rotary.layers_by_name["embeddings"].conf.paramKeys()
    assert learned.numParams() - rotary.numParams() == 16 * E
    assert all(rotary.layers_by_name[f"decoder_{i}"].conf.rotary() for i in range(2))
    assert "positionEmbeddings" not in learned.conf.toJson() and "positionEncoding" not in learned.conf.toJson()
    # one training step runs and moves every parameter block of the embedding
    x = _tokens()
    y = torch.zeros(MB, V, T)
    y.scatter_(1, torch.randint(0, V, (MB, 1, T), generator=torch.Generator().manual_seed(2)), 1.0)
    p0 = rotary.params().clone()
    rotary.fit([x], [y])
    assert torch.isfinite(rotary.params()).all() and not torch.equal(p0, rotary.params())


def test_rotary_generates_past_max_positions_and_learned_positions_refuse():
    prompt = _tokens(t=4, seed=9)
    learned, rotary = _zoo(False).init(device="cpu"), _zoo(True).init(device="cpu")
    learned.rnnClearPreviousState()
    learned.rnnTimeStep(_tokens(t=16, seed=8))
    with pytest.raises(DL4JInvalidInputException, match="maxPositions 16"):
        learned.rnnTimeStep(prompt[:, :1])                                   # the 17th token
    res = rotary.generate(prompt, maxNewTokens=40)
    assert res.tokens.shape == (MB, 40)
    pinned = rotary.generate(prompt, maxNewTokens=40, pinPositions=True)
    assert torch.equal(pinned.tokens, res.tokens)
    assert (pinned.scores - res.scores).abs().max() < 1e-4
    # and the hand loop on rnnTimeStep gives the same greedy tokens
    rotary.rnnClearPreviousState()
    p = rotary.rnnTimeStep(prompt)[0][:, :, -1]
    for t in range(40):
        tok = p.argmax(1)
        assert torch.equal(tok, res.tokens[:, t])
        p = rotary.rnnTimeStep(tok.reshape(MB, 1))[0][:, :, -1]
