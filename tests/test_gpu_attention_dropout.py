"""Dropout of the transformer block on the GPU: the in-kernel attention-dropout mask against the host oracle, the DROP
instances of the flash kernels against fp32 autograd with the oracle's mask, the LayerNorm forward with fused hidden
dropout and its backward chain, a tiny BERT against the CPU reference fed the GPU's masks, HIP-graph replays drawing
fresh masks, and the dropout-off path staying bit-identical."""
import functools

import pytest
import torch

from deeplearning4j_amd.ops import nn_misc
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

SEED = 0x5DEECE66D1234567


def _err(a, b):
    """The error measure of tests/test_gpu_transformer.py."""
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def _stream(cuda, offset=1, seed=SEED):
    st = nn_misc.PhiloxStream(cuda)
    st.seed = seed
    st.offset.fill_(offset)
    return st


@functools.lru_cache(maxsize=None)
def _oracle(offset, B, H, T, drop, seed=SEED):
    return TN.attn_dropout_keep(seed, offset, B, H, T, drop)


# ------------------------------------------------------------------------------------------------ 1. mask kernel
@pytest.mark.parametrize("offset", [1, 0x1_0000_0007])
@pytest.mark.parametrize("drop", [0.1, 0.5])
def test_mask_kernel_matches_oracle_bitwise(cuda, offset, drop):
    B, T, H = 2, 77, 3
    got = TN.attn_drop_mask(_stream(cuda, offset), B, H, T, drop).cpu()
    want = _oracle(offset, B, H, T, drop)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    thr, keep_eff = TN.attn_drop_threshold(drop)
    assert abs(got.float().mean().item() - keep_eff) < 0.02      # sigma ~ 0.004 for 35,574 draws at drop 0.5


# ------------------------------------------------------------------------------------------------ 2. flash kernels
_CASES = [(B, T, H, D, masked, causal, dt, 0.1)
          for (B, T, H, D) in [(2, 64, 2, 64), (3, 77, 4, 64), (2, 200, 2, 64), (2, 200, 2, 128)]
          for masked in (False, True) for causal in (False, True) for dt in (torch.bfloat16, torch.float16)]
_CASES.append((3, 77, 4, 64, True, False, torch.bfloat16, 0.5))


@pytest.mark.parametrize("B,T,H,D,masked,causal,dt,drop", _CASES)
def test_attention_dropout_fwd_bwd_matches_reference(cuda, B, T, H, D, masked, causal, dt, drop):
    """Tolerances and error measure of test_gpu_transformer.py::test_attention_fwd_bwd_matches_reference. A mask that
    differs in any one of the three kernels is an O(1) error in out, dV or dQ/dK."""
    g = torch.Generator().manual_seed(B * 1000 + T + D)
    qkv = (torch.randn(B, T, 3 * H * D, generator=g) * 0.8).to(dt)
    mask = None
    if masked:
        lens = torch.randint(T // 2, T + 1, (B,), generator=g)
        mask = (torch.arange(T).reshape(1, T) < lens.reshape(B, 1)).float()
    dout = torch.randn(B, T, H * D, generator=g).to(dt)
    _, keep_eff = TN.attn_drop_threshold(drop)
    keep = _oracle(1, B, H, T, drop).float() / keep_eff
    qr = qkv.float().requires_grad_(True)
    o_ref = TN.attention_reference(qr, H, mask, causal, keep=keep)
    o_ref.backward(dout.float())
    qd = qkv.to(cuda)
    md = mask.to(cuda) if mask is not None else None
    st = _stream(cuda, 1)
    out, lse = TN.attn_fwd(qd, H, md, causal, dropout=drop, rng=st)
    assert out.dtype == dt
    e = _err(out, o_ref.detach())
    print("fwd", e)
    assert e < 2e-2
    _, lse0 = TN.attn_fwd(qd, H, md, causal)
    assert (lse - lse0).abs().max().item() < 1e-6                # lse never sees the mask
    dqkv = TN.attn_bwd(qd, out, lse, dout.to(cuda), H, md, causal, dropout=drop, rng=st)
    E = H * D
    for name, sl in (("dQ", slice(0, E)), ("dK", slice(E, 2 * E)), ("dV", slice(2 * E, 3 * E))):
        e = _err(dqkv[..., sl], qr.grad[..., sl])
        print(name, e)
        assert e < 3e-2, (name, e)
    # the undropped reference is far away: the comparison above does see the mask
    assert _err(out, TN.attention_reference(qkv.float(), H, mask, causal)) > 2e-2


def test_fully_masked_rows_give_zero_output_and_gradient(cuda):
    B, T, H, D = 2, 70, 2, 64
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16).to(cuda)
    dout = torch.randn(B, T, H * D, generator=g).to(torch.bfloat16).to(cuda)
    mask = torch.ones(B, T, device=cuda)
    mask[1] = 0                                                   # every key of sequence 1 is padding
    st = _stream(cuda, 3)
    out, lse = TN.attn_fwd(qkv, H, mask, False, dropout=0.1, rng=st)
    dqkv = TN.attn_bwd(qkv, out, lse, dout, H, mask, False, dropout=0.1, rng=st)
    assert not out[1].any() and not dqkv[1].any()
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()


# ------------------------------------------------------------------------------------------------ 3. LayerNorm
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 2e-2), (torch.float16, 4e-3)])
@pytest.mark.parametrize("M,N", [(5, 64), (37, 1032), (1000, 768)])
def test_layernorm_fused_dropout_fwd_and_bwd_chain(cuda, dtype, tol, M, N):
    """Forward: the fused kernel against LN(dropout_native(x) + r) (1e-5 for fp32; for the 16-bit types the forward
    bound of the existing LayerNorm test, since the two sides round the dropped x at different points). Backward chain
    ln_bwd -> dropout backward -> column sums against fp32 autograd of layer_norm(keep*x + r), at the bounds
    test_layernorm_fwd_bwd_matches_reference uses for dx and for its column-sum outputs (dgamma / dbeta)."""
    drop = 0.1
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, N, generator=g) * 2 + 0.5).to(dtype)
    r = torch.randn(M, N, generator=g).to(dtype)
    gamma = torch.rand(N, generator=g) + 0.5
    beta = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g).to(dtype)
    xd, rd, gd, bd, dyd = (t.to(cuda) for t in (x, r, gamma, beta, dy))
    st = _stream(cuda, 5)
    y, mean, rstd, xdrop = TN.ln_fwd_dropout(xd, gd, bd, 1e-12, rd, drop, st)
    assert torch.equal(xd.cpu(), x)                               # not in place unless asked
    x_two = nn_misc.dropout_native(xd, "dropout", st, False, p=1.0 - drop)
    y_two, _, _ = TN.ln_fwd(x_two, gd, bd, 1e-12, rd)
    assert torch.equal(xdrop, x_two)                              # the same mask, the same rounding of x / keep
    e = _err(y, y_two)
    print("fwd", e)
    assert e < (1e-5 if dtype == torch.float32 else tol * 4)
    frac = (xdrop == 0).float().mean().item()
    assert abs(frac - drop) < 4 * (drop * (1 - drop) / (M * N)) ** 0.5 + 1e-3
    # in place: the same results, x overwritten with the dropped values
    xin = xd.clone()
    y_in, _, _, x_in = TN.ln_fwd_dropout(xin, gd, bd, 1e-12, rd, drop, st, inplace=True)
    assert x_in.data_ptr() == xin.data_ptr() and torch.equal(xin, xdrop) and torch.equal(y_in, y)
    # backward chain against autograd with the kernel's keep mask
    keep = nn_misc.dropout_native(torch.ones(M, N, device=cuda), "dropout", st, False, p=1.0 - drop).cpu()
    xr, rr = x.float().requires_grad_(True), r.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y_ref = torch.nn.functional.layer_norm(keep * xr + rr, (N,), gr, br, 1e-12)
    y_ref.backward(dy.float())
    assert _err(y, y_ref.detach()) < tol * 4
    ds, dg, db = TN.ln_bwd(dyd, xdrop, gd, mean, rstd, rd)
    dx = nn_misc.dropout_native(ds, "dropout", st, True, p=1.0 - drop)
    from deeplearning4j_amd.ops import native
    dsum = native.channel_sum(dx.contiguous())
    wide = 1 if dtype == torch.float32 else 4
    errs = {"dr": _err(ds, rr.grad), "dx": _err(dx, xr.grad), "dg": _err(dg, gr.grad), "db": _err(db, br.grad),
            "dsum": _err(dsum, xr.grad.sum(0))}
    print(errs)
    assert errs["dr"] < tol * 8 and errs["dx"] < tol * 8
    assert errs["dg"] < tol * 8 * wide and errs["db"] < tol * 8 * wide and errs["dsum"] < tol * 8 * wide


# ------------------------------------------------------------------------------------------------ 4. encoder stack
_BERT = dict(numLabels=3, inputShape=[40], vocabSize=97, hidden=128, layers=2, heads=2, ffn=256, maxPositions=64)


def _feed_gpu_masks(ref, gpu, cuda):
    """Make every dropout site of the CPU reference net use the mask the GPU net drew at its current step."""
    def keep_from(gimpl):
        def keep(site, shape, drop, like):
            st = gimpl.dropoutStream(site)
            if site == "attention":
                B, H, T, _ = shape
                _, keep_eff = TN.attn_drop_threshold(drop)
                return TN.attn_dropout_keep(st.seed, int(st.offset.item()), B, H, T, drop).float() / keep_eff
            ones = torch.ones(tuple(shape), device=cuda)
            return nn_misc.dropout_native(ones, "dropout", st, False, p=1.0 - drop).cpu()
        return keep
    for name in ["embeddings"] + [f"encoder_{i}" for i in range(_BERT["layers"])]:
        ref.getLayer(name).dropoutKeep = keep_from(gpu.getLayer(name))
    # the classifier's dropout is the reference-style IDropout object: same kernel, same mapping
    gdrop, rdrop = gpu.getLayer("classifier").conf.idropout, ref.getLayer("classifier").conf.idropout
    state = {}

    def apply(x, *a, **k):
        ones = torch.ones(tuple(x.shape), device=cuda)
        state["m"] = nn_misc.dropout_native(ones, "dropout", gdrop._rng, False, p=gdrop.p).cpu()
        return x * state["m"]
    rdrop.applyDropout = apply
    rdrop.backprop = lambda grad: grad * state["m"]


def test_bert_with_dropout_gpu_bf16_matches_cpu_fp32_with_the_same_masks(cuda):
    """The configuration and bounds of test_bert_block_gpu_bf16_matches_cpu_fp32, dropout 0.1 at every site."""
    from deeplearning4j_amd.models import BertBase
    from deeplearning4j_amd.nn.conf import DataType
    from deeplearning4j_amd.ops import fallback
    kw = dict(_BERT, hiddenDropout=0.1, attentionDropout=0.1, classifierDropout=0.1)
    ref = BertBase(**kw).init(device="cpu")
    gpu = BertBase(dataType=DataType.BFLOAT16, **kw).init(device=cuda)
    gpu.setParams(ref.params().to(cuda))
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 97, (6, 40), generator=g)
    y = torch.nn.functional.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float()
    m = torch.ones(6, 40)
    m[2, 25:] = 0
    fallback.reset()
    out_r = ref.output(x, masks=[m])[0]
    out_g = gpu.output(x.to(cuda), masks=[m.to(cuda)])[0]
    assert _err(out_g, out_r) < 3e-2
    gpu.computeGradientAndScore([x.to(cuda)], [y.to(cuda)], [m.to(cuda)])
    torch.cuda.synchronize()
    _feed_gpu_masks(ref, gpu, cuda)
    ref.computeGradientAndScore([x], [y], [m])
    gr, gg = ref.getGradientsViewArray().reshape(-1), gpu.getGradientsViewArray().reshape(-1).cpu()
    rel = ((gg - gr).norm() / gr.norm()).item()
    print("gradient rel", rel, "scores", float(gpu.score()), float(ref.score()))
    assert rel < 5e-2, rel
    assert abs(float(gpu.score()) - float(ref.score())) < 3e-2 * max(1.0, abs(float(ref.score())))
    assert gpu.helperCountFail() == 0
    # the masks matter: without them the reference is far away
    plain = BertBase(**_BERT).init(device="cpu")
    plain.setParams(ref.params())
    plain.computeGradientAndScore([x], [y], [m])
    gp = plain.getGradientsViewArray().reshape(-1)
    assert ((gg - gp).norm() / gp.norm()).item() > 0.2


# ------------------------------------------------------------------------------------------------ 5. HIP graphs
def _five_scores(cuda, graph):
    from deeplearning4j_amd.models import BertBase
    from deeplearning4j_amd.nn.conf import DataType
    torch.manual_seed(4321)
    net = BertBase(dataType=DataType.BFLOAT16, learningRate=0.0, hiddenDropout=0.1, attentionDropout=0.1,
                   classifierDropout=0.1, **_BERT).init(device=cuda)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 97, (6, 40), generator=g).to(cuda)
    y = torch.nn.functional.one_hot(torch.randint(0, 3, (6,), generator=g), 3).float().to(cuda)
    if graph:
        net.enableHipGraphs(True, warmup=2)
    torch.manual_seed(1234)
    scores = []
    for _ in range(5):
        net.fit([x], [y])
        scores.append(float(net.score()))
    return scores, net


def test_hip_graph_replays_draw_fresh_masks(cuda):
    """Zero learning rate and one fixed batch: the scores of consecutive steps differ through the masks alone. Two
    eager warm-up steps, then three replays of the captured step, against the same five steps run eagerly."""
    sg, net = _five_scores(cuda, True)
    captured = [c for c in getattr(net, "_hipgraphs", {}).values() if getattr(c, "ok", False)]
    assert captured and captured[0].k == 3, "the last three steps were not graph replays"
    se, _ = _five_scores(cuda, False)
    print("graph", sg, "eager", se)
    assert len({round(s, 6) for s in sg[2:]}) > 1                 # not all equal: a new mask per replay
    for a, b in zip(sg, se):
        assert abs(a - b) <= 1e-2 * max(abs(b), 1e-6), (sg, se)


# ------------------------------------------------------------------------------------------------ 6. default path
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_dropout_zero_is_the_path_without_the_arguments(cuda, dt):
    B, T, H, D = 2, 200, 2, 64
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(dt).to(cuda)
    dout = torch.randn(B, T, H * D, generator=g).to(dt).to(cuda)
    mask = torch.ones(B, T, device=cuda)
    mask[1, 150:] = 0
    out0, lse0 = TN.attn_fwd(qkv, H, mask, True)
    out1, lse1 = TN.attn_fwd(qkv, H, mask, True, dropout=0.0, rng=None)
    out2, lse2 = TN.attn_fwd(qkv, H, mask, True, dropout=0.0, rng=_stream(cuda))
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1) and torch.equal(out0, out2) and torch.equal(lse0, lse2)
    d0 = TN.attn_bwd(qkv, out0, lse0, dout, H, mask, True)
    d1 = TN.attn_bwd(qkv, out0, lse0, dout, H, mask, True, dropout=0.0, rng=None)
    assert torch.equal(d0, d1)
    with pytest.raises(ValueError):
        TN.attn_fwd(qkv, H, mask, True, dropout=0.1)              # a mask needs an rng
    with pytest.raises(ValueError):
        TN.attn_fwd(qkv, H, mask, True, dropout=1.0, rng=_stream(cuda))


def test_flash_attention_autograd_function_with_and_without_dropout(cuda):
    B, T, H, D = 2, 70, 2, 64
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16).to(cuda)
    dout = torch.randn(B, T, H * D, generator=g).to(torch.bfloat16).to(cuda)
    st = _stream(cuda, 2)
    for extra in ((), (0.1, st)):
        q = qkv.clone().requires_grad_(True)
        out = TN.FlashAttention.apply(q, H, None, False, *extra)
        out.backward(dout)
        kw = dict(dropout=extra[0], rng=extra[1]) if extra else {}
        o2, lse = TN.attn_fwd(qkv, H, None, False, **kw)
        assert torch.equal(out.detach(), o2)
        assert torch.equal(q.grad, TN.attn_bwd(qkv, o2, lse, dout, H, None, False, **kw))
