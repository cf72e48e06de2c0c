"""Dropout of the transformer block (CPU): the Philox host oracle of the attention-dropout mask, the explicit
attention path with a keep mask against fp64 autograd, an fp64 central-difference check of the encoder block with
hidden + attention dropout, and the public semantics (0 = today's path, training only, fresh masks per forward,
config validation, JSON, importBert)."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException
from deeplearning4j_amd.models import BertBase
from deeplearning4j_amd.ops import transformer_native as TN


# ------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """Random123 known-answer vectors of Philox-4x32-10."""
    assert " ".join("%08x" % w for w in TN.philox4x32_10(ctr, key)) == want


@functools.lru_cache(maxsize=None)
def _keep(seed, offset, B, H, T, drop):
    return TN.attn_dropout_keep(seed, offset, B, H, T, drop)


def test_oracle_statistics_and_independence():
    seed, B, H, T, drop = 0x1234567890ABCDEF, 2, 2, 128, 0.1
    k = _keep(seed, 1, B, H, T, drop)
    assert k.shape == (B, H, T, T) and k.dtype == torch.uint8
    thr, keep_eff = TN.attn_drop_threshold(drop)
    assert thr == 26 and abs(keep_eff - (1 - 26 / 256)) < 1e-12
    dropped = 1.0 - k.float().mean().item()
    assert abs(dropped - (1.0 - keep_eff)) < 0.01, dropped        # sigma ~ 0.0012 for 65,536 draws
    assert torch.equal(k, TN.attn_dropout_keep(seed, 1, B, H, T, drop))          # deterministic
    assert not torch.equal(k, _keep(seed, 2, B, H, T, drop))                     # another step
    assert not torch.equal(k, _keep(seed + 1, 1, B, H, T, drop))                 # another seed
    assert not torch.equal(k, _keep(seed ^ (1 << 40), 1, B, H, T, drop))         # the high key word counts too
    flat = k.reshape(B * H, T, T)
    for i in range(B * H):
        for j in range(i + 1, B * H):
            assert not torch.equal(flat[i], flat[j])                             # another b*H + h
    # tiling independence: a shorter sequence sees the top-left corner of the same mask
    assert torch.equal(_keep(seed, 1, B, H, 77, drop), k[:, :, :77, :77])


# ------------------------------------------------------------------------------------------------ explicit path
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_explicit_attention_with_keep_matches_autograd(masked, causal):
    B, T, H, D = 2, 9, 2, 8
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(B, T, 3 * H * D, generator=g, dtype=torch.float64)
    dout = torch.randn(B, T, H * D, generator=g, dtype=torch.float64)
    mask = None
    if masked:
        mask = torch.ones(B, T, dtype=torch.float64)
        mask[0, 6:] = 0
        mask[1, 3:] = 0
    keep = (torch.rand(B, H, T, T, generator=g) < 0.75).double() / 0.75
    ref_in = qkv.clone().requires_grad_(True)
    ref = TN.attention_reference(ref_in, H, mask, causal, keep=keep)
    ref.backward(dout)
    out, ctx = TN.attention_fwd_explicit(qkv, H, mask, causal, keep=keep)
    dqkv = TN.attention_bwd_explicit(ctx, dout, qkv.dtype)

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()
    assert rel(out, ref.detach()) < 1e-9
    assert rel(dqkv, ref_in.grad) < 1e-9
    # and the mask matters
    assert rel(TN.attention_fwd_explicit(qkv, H, mask, causal)[0], ref.detach()) > 1e-3


# ------------------------------------------------------------------------------------------------ encoder block
def _block(E=16, H=2, F=32, T=5, dtype=None, **drops):
    b = TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F)
    for k, v in drops.items():
        b = getattr(b, k)(v)
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(dtype or DataType.DOUBLE).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.5)).graphBuilder())
    g.addInputs("x")
    g.addLayer("enc", b.build(), "x")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MSE).activation(Activation.IDENTITY).nIn(E).nOut(E).build(),
               "enc")
    g.setOutputs("out")
    g.setInputTypes(InputType.recurrent(E, T))
    net = ComputationGraph(g.build())
    net.init(device="cpu")
    return net


def _enc(net):
    return net.getLayer("enc")


def test_encoder_block_gradients_with_dropout_fp64():
    """Central differences on 200 randomly chosen parameters, on bo / b2, and on every input element against
    backpropGradient, the masks fixed by reseeding torch's generator before every forward. Tolerances: those of
    checkGradients as tests/test_transformer.py uses it (epsilon 1e-6, max relative error 1e-3, minimum absolute
    error 1e-8). A bias gradient summed over ds instead of ds∘D, or a residual gradient that sees the mask, fails
    here."""
    E, T, mb = 16, 5, 3
    net = _block(E=E, H=2, F=32, T=T, attentionDropout=0.25, hiddenDropout=0.25)
    impl = _enc(net)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(mb, E, T, generator=g, dtype=torch.float64)
    w = torch.randn(mb, E, T, generator=g, dtype=torch.float64)
    mask = torch.ones(mb, T, dtype=torch.float64)
    mask[1, 3:] = 0

    def loss(xin):
        torch.manual_seed(99)
        return float((impl.activate(xin, training=True, mask=mask) * w).sum())

    loss(x)
    _, dx = impl.backpropGradient(w)
    dx = dx.clone()
    analytic = {k: v.clone() for k, v in impl.grads.items()}
    flat = [(k, i) for k, v in impl.params.items() for i in range(v.numel())]
    pick = torch.randperm(len(flat), generator=g)[:200].tolist()
    # ... plus every element of the two bias gradients that follow a dropout site (32 values; few of them are drawn)
    pick = sorted(set(pick) | {j for j, (k, _) in enumerate(flat) if k in ("bo", "b2")})
    eps, fails, worst = 1e-6, [], 0.0

    def check(name, an, num):
        nonlocal worst
        denom = abs(an) + abs(num)
        rel = 0.0 if denom == 0 else abs(an - num) / denom
        if rel > 1e-3 and abs(an - num) > 1e-8:
            fails.append((name, an, num, rel))
        elif abs(an - num) > 1e-8:
            worst = max(worst, rel)

    with torch.no_grad():
        for j in pick:
            k, i = flat[j]
            p = impl.params[k].view(-1)
            orig = p[i].item()
            p[i] = orig + eps
            sp = loss(x)
            p[i] = orig - eps
            sm = loss(x)
            p[i] = orig
            check(f"{k}[{i}]", analytic[k].reshape(-1)[i].item(), (sp - sm) / (2 * eps))
        xf = x.reshape(-1)
        for i in range(xf.numel()):
            orig = xf[i].item()
            xf[i] = orig + eps
            sp = loss(x)
            xf[i] = orig - eps
            sm = loss(x)
            xf[i] = orig
            check(f"x[{i}]", dx.reshape(-1)[i].item(), (sp - sm) / (2 * eps))
    print(f"dropout gradient check: {len(pick) + xf.numel()} values, {len(fails)} failed, worst rel {worst:.3e}")
    assert {k for k, _ in (flat[j] for j in pick)} >= {"bo", "b2", "Wo", "W2", "Wqkv"}
    assert not fails, fails[:10]


# ------------------------------------------------------------------------------------------------ semantics
def _fwd_bwd(net, x, w, training=True, seed=5):
    impl = _enc(net)
    torch.manual_seed(seed)
    y = impl.activate(x, training=training).clone()
    if not training:
        return y, None, None
    _, dx = impl.backpropGradient(w)
    return y, dx.clone(), {k: v.clone() for k, v in impl.grads.items()}


def _xw(E=16, T=5, mb=3):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(mb, E, T, generator=g, dtype=torch.float64),
            torch.randn(mb, E, T, generator=g, dtype=torch.float64))


def test_zero_probabilities_are_todays_path_bit_for_bit():
    x, w = _xw()
    plain = _block()
    zero = _block(attentionDropout=0.0, hiddenDropout=0.0)
    zero.setParams(plain.params())
    y0, dx0, g0 = _fwd_bwd(plain, x, w)
    y1, dx1, g1 = _fwd_bwd(zero, x, w)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert _enc(zero)._drop_rng is None                  # no RNG state is even created


def test_hidden_dropout_is_applied_in_training_only():
    x, w = _xw()
    plain = _block()
    drop = _block(hiddenDropout=0.5)
    drop.setParams(plain.params())
    y_plain, _, _ = _fwd_bwd(plain, x, w)
    y_drop, _, _ = _fwd_bwd(drop, x, w)
    assert not torch.allclose(y_plain, y_drop)           # the field used to be ignored
    y_eval_plain, _, _ = _fwd_bwd(plain, x, w, training=False)
    y_eval_drop, _, _ = _fwd_bwd(drop, x, w, training=False)
    assert torch.equal(y_eval_plain, y_eval_drop)
    assert torch.equal(drop.outputSingle(x), plain.outputSingle(x))


def test_attention_dropout_is_applied_in_training_only():
    x, w = _xw()
    plain = _block()
    drop = _block(attentionDropout=0.5)
    drop.setParams(plain.params())
    assert not torch.allclose(_fwd_bwd(plain, x, w)[0], _fwd_bwd(drop, x, w)[0])
    assert torch.equal(_fwd_bwd(plain, x, w, training=False)[0], _fwd_bwd(drop, x, w, training=False)[0])


def test_consecutive_training_forwards_draw_new_masks():
    x, _ = _xw()
    impl = _enc(_block(hiddenDropout=0.3, attentionDropout=0.3))
    torch.manual_seed(0)
    y1 = impl.activate(x, training=True).clone()
    y2 = impl.activate(x, training=True).clone()
    assert not torch.allclose(y1, y2)
    assert int(impl._drop_rng.offset.item()) == 2        # one advance per training forward


def test_self_attention_and_embedding_layers_drop_in_training_only():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 5, generator=g)
    conf = SelfAttentionLayer.Builder().nIn(8).nOut(8).nHeads(2).attentionDropout(0.5) \
        .activation(Activation.IDENTITY).build()
    net = MultiLayerNetwork(NeuralNetConfiguration.Builder().seed(1).list().layer(0, conf).layer(
        1, RnnOutputLayer.Builder(LossFunction.MSE).activation(Activation.IDENTITY).nIn(8).nOut(8).build())
        .setInputType(InputType.recurrent(8, 5)).build())
    net.init()
    impl = net.getLayer(0)
    e1, e2 = impl.activate(x, training=False).clone(), impl.activate(x, training=False).clone()
    t1 = impl.activate(x, training=True).clone()
    assert torch.equal(e1, e2) and not torch.allclose(e1, t1)
    emb = BertBase(numLabels=2, inputShape=[6], vocabSize=20, hidden=8, layers=1, heads=2, ffn=16, maxPositions=8,
                   hiddenDropout=0.5).init(device="cpu").getLayer("embeddings")
    ids = torch.randint(0, 20, (3, 6), generator=g)
    ye = emb.activate(ids, training=False).clone()
    yt = emb.activate(ids, training=True).clone()
    assert (yt == 0).float().mean() > 0.25 and not (ye == 0).any()


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, "0.1", None])
def test_out_of_range_probabilities_are_refused(p):
    with pytest.raises(DL4JInvalidConfigException):
        TransformerEncoderLayer.Builder().nIn(8).nOut(8).nHeads(2).hiddenDropout(p).build()
    with pytest.raises(DL4JInvalidConfigException):
        TransformerEncoderLayer.Builder().nIn(8).nOut(8).nHeads(2).attentionDropout(p).build()
    with pytest.raises(DL4JInvalidConfigException):
        SelfAttentionLayer.Builder().nIn(8).nOut(8).nHeads(2).attentionDropout(p).build()
    with pytest.raises(DL4JInvalidConfigException):
        BertEmbeddingLayer.Builder().nIn(8).nOut(8).hiddenDropout(p).build()


def test_json_round_trip_and_legacy_config():
    import json
    conf = BertBase(numLabels=2, inputShape=[6], vocabSize=20, hidden=8, layers=1, heads=2, ffn=16, maxPositions=8,
                    hiddenDropout=0.1, attentionDropout=0.2, classifierDropout=0.3).conf()
    back = ComputationGraphConfiguration.fromJson(conf.toJson())
    assert back.toJson() == conf.toJson()

    def layer(c, name):
        lc = c.vertices[name].layerConf
        return getattr(lc, "layer", lc)
    assert layer(back, "encoder_0").hiddenDropout == 0.1 and layer(back, "encoder_0").attentionDropout == 0.2
    assert layer(back, "embeddings").hiddenDropout == 0.1
    assert abs(layer(back, "classifier").idropout.p - 0.7) < 1e-12          # retain probability
    # a config written before the fields existed: the keys are simply absent

    def strip(o):
        if isinstance(o, dict):
            return {k: strip(v) for k, v in o.items() if k not in ("hiddenDropout", "attentionDropout")}
        return [strip(v) for v in o] if isinstance(o, list) else o
    legacy = ComputationGraphConfiguration.fromJson(json.dumps(strip(json.loads(conf.toJson()))))
    assert layer(legacy, "encoder_0").hiddenDropout == 0.0 and layer(legacy, "encoder_0").attentionDropout == 0.0
    assert layer(legacy, "embeddings").hiddenDropout == 0.0
    enc = TransformerEncoderLayer.Builder().nIn(8).nOut(8).nHeads(2).build()
    assert enc.hiddenDropout == 0.0 and enc.attentionDropout == 0.0


def test_import_bert_dropout_argument():
    from deeplearning4j_amd.modelimport.bert import importBert
    E, F, V, P, L = 8, 16, 20, 8, 1
    cfg = {"vocab_size": V, "hidden_size": E, "num_hidden_layers": L, "num_attention_heads": 2,
           "intermediate_size": F, "max_position_embeddings": P, "hidden_dropout_prob": 0.1,
           "attention_probs_dropout_prob": 0.2, "classifier_dropout": None}
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g) * 0.1  # noqa: E731
    sd = {"embeddings.word_embeddings.weight": r(V, E), "embeddings.position_embeddings.weight": r(P, E),
          "embeddings.token_type_embeddings.weight": r(2, E), "embeddings.LayerNorm.weight": r(E),
          "embeddings.LayerNorm.bias": r(E), "pooler.dense.weight": r(E, E), "pooler.dense.bias": r(E),
          "classifier.weight": r(2, E), "classifier.bias": r(2)}
    p = "encoder.layer.0."
    for n in ("query", "key", "value"):
        sd[p + f"attention.self.{n}.weight"], sd[p + f"attention.self.{n}.bias"] = r(E, E), r(E)
    sd.update({p + "attention.output.dense.weight": r(E, E), p + "attention.output.dense.bias": r(E),
               p + "attention.output.LayerNorm.weight": r(E), p + "attention.output.LayerNorm.bias": r(E),
               p + "intermediate.dense.weight": r(F, E), p + "intermediate.dense.bias": r(F),
               p + "output.dense.weight": r(E, F), p + "output.dense.bias": r(E),
               p + "output.LayerNorm.weight": r(E), p + "output.LayerNorm.bias": r(E)})

    def probs(net):
        enc, emb, cls = (net.getLayer(n).conf for n in ("encoder_0", "embeddings", "classifier"))
        return enc.hiddenDropout, enc.attentionDropout, emb.hiddenDropout, \
            (0.0 if cls.idropout is None else round(1.0 - cls.idropout.p, 12))
    assert probs(importBert(sd, cfg, seqLen=6, device="cpu")) == (0.0, 0.0, 0.0, 0.0)
    assert probs(importBert(sd, cfg, seqLen=6, device="cpu", dropout="config")) == (0.1, 0.2, 0.1, 0.1)
    assert probs(importBert(sd, dict(cfg, classifier_dropout=0.4), seqLen=6, device="cpu", dropout="config")) == \
        (0.1, 0.2, 0.1, 0.4)
    assert probs(importBert(sd, cfg, seqLen=6, device="cpu", dropout=0.25)) == (0.25, 0.25, 0.25, 0.25)
    ids = torch.randint(0, V, (2, 6), generator=g)
    a = importBert(sd, cfg, seqLen=6, device="cpu").output(ids)[0]
    b = importBert(sd, cfg, seqLen=6, device="cpu", dropout="config").output(ids)[0]
    assert torch.equal(a, b)                              # inference does not see the dropout
