"""Cross-attention HIP kernels (csrc/attention_cross.hip) against the plain-torch fp32 reference on the rounded inputs,
with the normalised max error and the bounds of tests/test_gpu_transformer.py (the same arithmetic): every block
edge on the query and the key axis independently, key-padding masks, a fully masked batch row, a kv buffer with
spare capacity, refusals, bitwise determinism; then the decoder block as a graph layer in bf16 against the same
weights in fp32 on the CPU, token-by-token generation, and the kernels one decode step launches."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = [(1, 1), (1, 64), (1, 65), (17, 63), (64, 128), (65, 1), (70, 130), (3, 200)]


def _err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def _operands(B, Tq, Tk, H, D, dt, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + B * 1000 + Tq * 31 + Tk + D)
    E = H * D
    q = (torch.randn(B, Tq, E, generator=g) * 0.8).to(dt)
    kv = (torch.randn(B, Tk, 2 * E, generator=g) * 0.8).to(dt)
    dout = torch.randn(B, Tq, E, generator=g).to(dt)
    return q, kv, dout


def _ragged(B, Tk):
    """Key-padding mask of ragged lengths; the last batch row keeps a single key."""
    lens = [max(1, Tk - 1 - 3 * b) for b in range(B)]
    lens[-1] = 1
    return (torch.arange(Tk).reshape(1, Tk) < torch.tensor(lens).reshape(B, 1)).float()


def _reference(q, kv, dout, H, kmask):
    qr, kr = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    o = TN.cross_attention_reference(qr, kr, H, kmask)
    o.backward(dout.float())
    return o.detach(), qr.grad, kr.grad


@pytest.mark.parametrize("Tq,Tk", SHAPES)
@pytest.mark.parametrize("B,H,D", [(2, 2, 64), (1, 3, 128)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_cross_fwd_bwd_matches_reference(B, H, D, Tq, Tk, masked, dt):
    q, kv, dout = _operands(B, Tq, Tk, H, D, dt)
    kmask = _ragged(B, Tk) if masked else None
    o_ref, dq_ref, dkv_ref = _reference(q, kv, dout, H, kmask)
    qd, kvd = q.to(DEV), kv.to(DEV)
    md = kmask.to(DEV) if masked else None
    out, lse = TN.cross_attn_fwd(qd, kvd, H, kmask=md)
    assert out.dtype == dt and out.shape == (B, Tq, H * D) and lse.shape == (B, H, Tq)
    e = _err(out, o_ref)
    print(f"fwd {e:.3e}")
    assert e < 2e-2, e
    dq, dkv = TN.cross_attn_bwd(qd, kvd, out, lse, dout.to(DEV), H, kmask=md)
    assert dq.shape == q.shape and dkv.shape == kv.shape
    E = H * D
    for name, a, b in (("dQ", dq, dq_ref), ("dK", dkv[..., :E], dkv_ref[..., :E]), ("dV", dkv[..., E:], dkv_ref[..., E:])):
        e = _err(a, b)
        print(f"{name} {e:.3e}")
        assert torch.isfinite(a).all(), name
        assert e < 3e-2, (name, e)


@pytest.mark.parametrize("B,H,D,Tq,Tk", [(3, 2, 64, 17, 70), (2, 2, 128, 65, 5)])
def test_fully_masked_batch_row_gives_zeros_and_finite_gradients(B, H, D, Tq, Tk):
    dt = torch.bfloat16
    q, kv, dout = _operands(B, Tq, Tk, H, D, dt, seed=1)
    kmask = _ragged(B, Tk)
    kmask[0] = 0
    o_ref, dq_ref, dkv_ref = _reference(q, kv, dout, H, kmask)
    out, lse = TN.cross_attn_fwd(q.to(DEV), kv.to(DEV), H, kmask=kmask.to(DEV))
    dq, dkv = TN.cross_attn_bwd(q.to(DEV), kv.to(DEV), out, lse, dout.to(DEV), H, kmask=kmask.to(DEV))
    for t in (out, lse, dq, dkv):
        assert torch.isfinite(t).all()
    assert out[0].abs().max() == 0 and dq[0].abs().max() == 0 and dkv[0].abs().max() == 0
    assert (lse[0] == 1e30).all()
    assert _err(out, o_ref) < 2e-2 and _err(dq, dq_ref) < 3e-2 and _err(dkv, dkv_ref) < 3e-2


@pytest.mark.parametrize("D,Tq,Tk,cap", [(64, 5, 70, 128), (128, 66, 3, 64), (64, 1, 130, 200)])
def test_rows_beyond_tk_are_never_read(D, Tq, Tk, cap):
    B, H, dt = 2, 2, torch.float16
    q, kv, dout = _operands(B, Tq, Tk, H, D, dt, seed=2)
    big = torch.full((B, cap, 2 * H * D), float("nan"), dtype=dt)
    big[:, :Tk] = kv
    kmask = _ragged(B, Tk).to(DEV)
    qd, dd = q.to(DEV), dout.to(DEV)
    out, lse = TN.cross_attn_fwd(qd, kv.to(DEV), H, kmask=kmask)
    dq, dkv = TN.cross_attn_bwd(qd, kv.to(DEV), out, lse, dd, H, kmask=kmask)
    out2, lse2 = TN.cross_attn_fwd(qd, big.to(DEV), H, Tk=Tk, kmask=kmask)
    dq2, dkv2 = TN.cross_attn_bwd(qd, big.to(DEV), out2, lse2, dd, H, kmask=kmask, Tk=Tk)
    assert torch.isfinite(out2).all() and torch.equal(out2, out) and torch.equal(lse2, lse)
    assert dkv2.shape == (B, Tk, 2 * H * D)
    assert torch.equal(dq2, dq) and torch.equal(dkv2, dkv)


def test_unsupported_operands_are_refused_and_nothing_is_written():
    def run(q, kv, H, Tk=None):
        assert not TN.cross_attn_supported(q, kv, H) or Tk is not None
        assert TN.cross_attn_fwd(q, kv, H, Tk=Tk) is None
        out, lse = torch.zeros_like(q), torch.zeros(q.shape[0], H, q.shape[1], device=q.device)
        assert TN.cross_attn_bwd(q, kv, out, lse, torch.zeros_like(q), H, Tk=Tk) is None

    B, Tq, Tk = 2, 5, 9
    run(torch.zeros(B, Tq, 2 * 32, device=DEV, dtype=torch.bfloat16),
        torch.zeros(B, Tk, 4 * 32, device=DEV, dtype=torch.bfloat16), 2)                       # head size 32
    run(torch.zeros(B, Tq, 128, device=DEV), torch.zeros(B, Tk, 256, device=DEV), 2)           # fp32
    flat = torch.zeros(B * Tq * 128 + 8, device=DEV, dtype=torch.bfloat16)
    run(flat[1:1 + B * Tq * 128].view(B, Tq, 128),
        torch.zeros(B, Tk, 256, device=DEV, dtype=torch.bfloat16), 2)                          # 2-byte aligned view
    run(torch.zeros(B, Tq, 128, device=DEV, dtype=torch.bfloat16),
        torch.zeros(B, Tk, 256, device=DEV, dtype=torch.bfloat16), 2, Tk=Tk + 1)               # Tk > TkCap
    # the C entry points themselves: -1 and untouched outputs
    from deeplearning4j_amd.ops import native
    from deeplearning4j_amd.ops.native import _ptr, _stream
    lib = native.load()
    q = torch.randn(B, Tq, 128, device=DEV).to(torch.bfloat16)
    kv = torch.randn(B, Tk, 256, device=DEV).to(torch.bfloat16)
    out = torch.full_like(q, 7.0)
    lse = torch.full((B, 2, Tq), 7.0, device=DEV)
    for dt_code, tk, cap, D, qq in ((1, Tk + 1, Tk, 64, q), (0, Tk, Tk, 64, q), (3, Tk, Tk, 64, q), (1, Tk, Tk, 32, q),
                                    (1, Tk, Tk, 64, q.view(-1)[1:])):
        rc = lib.dl4j_attn_cross_fwd_dt(dt_code, _ptr(qq), _ptr(kv), None, _ptr(out), _ptr(lse), B, Tq, tk, cap,
                                        128 // D, D, 0.125, _stream())
        assert rc == -1
    assert lib.dl4j_attn_cross_fwd_dt(1, _ptr(q), _ptr(kv), None, _ptr(out), _ptr(lse), 65536, Tq, Tk, Tk, 1, 64,
                                      0.125, _stream()) == -1                                  # B*H > 65535
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (lse == 7.0).all()


def test_forward_and_backward_are_bitwise_reproducible():
    B, H, D, Tq, Tk = 2, 2, 64, 70, 130
    q, kv, dout = (t.to(DEV) for t in _operands(B, Tq, Tk, H, D, torch.bfloat16, seed=3))
    kmask = _ragged(B, Tk).to(DEV)
    runs = []
    for _ in range(2):
        out, lse = TN.cross_attn_fwd(q, kv, H, kmask=kmask)
        dq, dkv = TN.cross_attn_bwd(q, kv, out, lse, dout, H, kmask=kmask)
        runs.append((out, lse, dq, dkv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("T", [1, 65, 130])                  # one row; one past a block edge; two blocks and a tail
@pytest.mark.parametrize("B,H,D", [(2, 2, 64), (1, 3, 128)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_cross_equals_self_attention_bitwise_at_equal_lengths(B, H, D, T, masked, dt):
    """The self and the cross kernels run one body (csrc/attention_body.h): at Tq = Tk = T with the same key-padding
    mask, non-causal and without dropout, they give the same bits on q | kv = qkv."""
    q, kv, dout = (t.to(DEV) for t in _operands(B, T, T, H, D, dt, seed=4))
    qkv = torch.cat([q, kv], 2).contiguous()
    md = _ragged(B, T).to(DEV) if masked else None
    E = H * D
    out, lse = TN.cross_attn_fwd(q, kv, H, kmask=md)
    s_out, s_lse = TN.attn_fwd(qkv, H, mask=md)
    assert torch.equal(out, s_out) and torch.equal(lse, s_lse)
    dq, dkv = TN.cross_attn_bwd(q, kv, out, lse, dout, H, kmask=md)
    dqkv = TN.attn_bwd(qkv, s_out, s_lse, dout, H, mask=md)
    assert torch.equal(dq, dqkv[..., :E])
    assert torch.equal(dkv, dqkv[..., E:])


# ------------------------------------------------------------------------------------------------ layer / network
EH, NH, FF, TS, TT, MB, V = 128, 2, 256, 70, 66, 3, 11


def _seq2seq(dt, device):
    from deeplearning4j_amd.models import TransformerSeq2Seq
    return TransformerSeq2Seq(numLabels=V, sourceVocabSize=13, inputShape=[TS, TT], hidden=EH, layers=2, heads=NH,
                              ffn=FF, maxPositions=TS + 2, dataType=dt).init(device=device)


@pytest.fixture(scope="module")
def nets():
    """(bf16 GPU net, fp32 CPU net with the same weights, source, target, source mask, CPU output): the CPU reference
    is computed once and left unchanged."""
    cpu = _seq2seq(DataType.FLOAT, "cpu")
    gpu = _seq2seq(DataType.BFLOAT16, DEV)
    gpu.setParams(cpu.params().to(DEV))
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 13, (MB, TS), generator=g)
    tgt = torch.randint(0, V, (MB, TT), generator=g)
    sm = torch.ones(MB, TS)
    sm[1, 40:] = 0
    sm[2, 5:] = 0
    ref = cpu.output(src, tgt, masks=[sm, None])[0].clone()
    return gpu, cpu, src, tgt, sm, ref


def test_decoder_graph_gpu_bf16_matches_cpu_fp32(nets):
    gpu, cpu, src, tgt, sm, ref = nets
    fallback.reset()
    out = gpu.output(src.to(DEV), tgt.to(DEV), masks=[sm.to(DEV), None])[0].cpu()
    rel = (out - ref).norm() / ref.norm()
    print(f"output rel L2 {rel:.3e}")
    assert rel < 3e-2, rel
    lab = torch.nn.functional.one_hot(torch.roll(tgt, -1, 1), V).permute(0, 2, 1).float()
    cpu.computeGradientAndScore([src, tgt], [lab], [sm, None])
    gpu.computeGradientAndScore([src.to(DEV), tgt.to(DEV)], [lab.to(DEV)], [sm.to(DEV), None])
    gr, gg = cpu.getGradientsViewArray().reshape(-1), gpu.getGradientsViewArray().reshape(-1).cpu()
    assert torch.isfinite(gg).all()
    relg = (gg - gr).norm() / gr.norm()
    print(f"flat gradient rel L2 {relg:.3e}")
    assert relg < 5e-2, relg
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()


def test_token_by_token_generation_matches_cpu_output(nets):
    gpu, cpu, src, tgt, sm, ref = nets
    fallback.reset()
    td = tgt.to(DEV)
    gpu.rnnClearPreviousState()
    ys = [gpu.rnnTimeStep(src.to(DEV), td[:, :1], masks=[sm.to(DEV), None])[0]]
    ys += [gpu.rnnTimeStep(None, td[:, t:t + 1])[0] for t in range(1, TT)]
    got = torch.cat(ys, 2).cpu()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    assert torch.isfinite(got).all()
    rel = (got - ref).norm() / ref.norm()
    print(f"rnnTimeStep bf16 GPU vs fp32 CPU output over {TT} steps: rel {rel:.3e}")
    assert rel < 3e-2, rel
    st = gpu.rnnGetPreviousState("decoder_1")
    assert st["mem_kv"].shape == (MB, TS, 2 * EH) and st["kv"].shape == (MB, TT, 2 * EH)


def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


# rnnTimeStep ends with ``.float()`` of the bf16 output layer's activations: the one torch launch of a decode step
_ALLOWED = ("bfloat16tofloat32_copy_kernel",)


def test_decode_step_runs_cross_kernel_per_block_and_no_encoder_or_torch_kernels():
    from torch.profiler import ProfilerActivity, profile
    from deeplearning4j_amd.models import TransformerSeq2Seq
    net = TransformerSeq2Seq(numLabels=77, inputShape=[16, 16], hidden=128, layers=2, heads=2, maxPositions=64,
                             dataType=DataType.BFLOAT16).init(device=DEV)
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 77, (4, 16), generator=g).to(DEV)
    x = torch.randint(0, 77, (4, 8), generator=g).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    net.rnnTimeStep(src, steps[0])                              # encoder + memory projections, kernel choices
    net.rnnTimeStep(None, steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(None, steps[2])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 10, names
    for n in names:
        print("  kernel:", n[:120])
    assert sum("attn_cross_fwd_kernel" in n for n in names) == 2          # once per decoder block
    assert sum("attn_decode_kernel" in n for n in names) == 2 and sum("attn_kv_append" in n for n in names) == 2
    assert not any("attn_fwd_kernel" in n for n in names)                 # no encoder attention
    assert sum("bert_embed" in n for n in names) == 1                     # the target's embedding only
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
