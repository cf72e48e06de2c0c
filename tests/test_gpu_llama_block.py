"""RMSNorm (csrc/rmsnorm.hip), SwiGLU (csrc/swiglu.hip) and the Llama-style block on the GPU, bf16 and fp16.

(a) the refusals of every entry point and wrapper; (b) ``rms_fwd`` against the fp64 formula on the same 16-bit inputs,
every element within one rounding, and the fused residual add bitwise against "add, round, norm"; (c) ``rms_bwd``
against fp64, its column sums, reproducibility and aliasing; (d) ``swiglu`` forward and backward against fp64 with
planted gates far out on both sides; (e) a two-block rms / pre / swiglu language model with rotary grouped heads: a
training step and generation against fp32 on the CPU, pinned and graph-replayed generation, the fp8 cache, ragged
prompts, and the kernels of one training step and one decode step.

The constants (unit roundoff ``U``, smallest subnormal ``TINY``, ``_err`` and its bound) are those of
tests/test_gpu_rope.py."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
DTS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
TOL = 2e-2
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}
EPS = 1e-5
NS = [64, 776, 4096]          # a wave that is mostly idle, a partly filled second chunk, the register maximum


def _err(a, b):
    """The error measure of tests/test_gpu_attention_decode.py."""
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def _bits(t):
    return t.cpu().view(torch.int16) if t.dtype in DTS else t.cpu().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _rows(dt, M, N, seed):
    """[M, N] on the CPU, never modified."""
    g = torch.Generator().manual_seed(100000 * seed + 10 * N + M)
    return (torch.randn(M, N, generator=g) * 1.5).to(dt)


@functools.lru_cache(maxsize=None)
def _gamma(N):
    g = torch.Generator().manual_seed(N)
    return 1.0 + 0.5 * torch.randn(N, generator=g)


def _rms64(s, gamma, eps=EPS):
    """The fp64 formula on the 16-bit values s -> (y, rstd [M, 1])."""
    s64 = s.double()
    rstd = torch.rsqrt((s64 * s64).mean(-1, keepdim=True) + eps)
    return s64 * rstd * gamma.double(), rstd


# ------------------------------------------------------------------------------------------------ (a) refusals
def test_the_entry_points_refuse():
    lib = TN._lib()
    p, s = TN._ptr, TN._stream()
    M, N = 4, 64
    buf = torch.zeros(M * 4104 + 64, dtype=torch.bfloat16, device=DEV)
    x, r, y, so = (torch.zeros_like(buf) for _ in range(4))
    g = torch.ones(4104, dtype=torch.float32, device=DEV)
    rstd = torch.zeros(M, dtype=torch.float32, device=DEV)
    part = torch.zeros(2 * 4104 * M, dtype=torch.float32, device=DEV)
    dg, dsum = torch.zeros(4104, dtype=torch.float32, device=DEV), torch.zeros(4104, dtype=torch.float32, device=DEV)
    off = lambda t: p(t[4:])  # noqa: E731  8 bytes past a 16-byte boundary
    fwd = lib.dl4j_rms_fwd
    assert fwd(1, p(x), None, p(g), p(y), None, p(rstd), M, N, EPS, s) == 0
    assert fwd(1, p(x), p(r), p(g), p(y), p(so), p(rstd), M, N, EPS, s) == 0
    assert fwd(1, p(x), p(r), p(g), p(y), p(x), p(rstd), M, N, EPS, s) == 0              # s_out aliases x
    assert fwd(1, p(x), None, p(g), p(y), None, p(rstd), M, 4104, EPS, s) == -1           # N > 4096
    assert fwd(1, p(x), None, p(g), p(y), None, p(rstd), M, 60, EPS, s) == -1             # N % 8
    assert fwd(1, p(x), None, p(g), p(y), None, p(rstd), 0, N, EPS, s) == -1              # M < 1
    assert fwd(3, p(x), None, p(g), p(y), None, p(rstd), M, N, EPS, s) == -1              # dtype
    assert fwd(1, p(x), None, p(g), p(y), p(so), p(rstd), M, N, EPS, s) == -1             # s_out without r
    assert fwd(1, None, None, p(g), p(y), None, p(rstd), M, N, EPS, s) == -1
    assert fwd(1, p(x), None, None, p(y), None, p(rstd), M, N, EPS, s) == -1
    assert fwd(1, p(x), None, p(g), None, None, p(rstd), M, N, EPS, s) == -1
    assert fwd(1, p(x), None, p(g), p(y), None, None, M, N, EPS, s) == -1
    assert fwd(1, off(x), None, p(g), p(y), None, p(rstd), M, N, EPS, s) == -1            # misaligned operands
    assert fwd(1, p(x), None, p(g), off(y), None, p(rstd), M, N, EPS, s) == -1
    assert fwd(1, p(x), off(r), p(g), p(y), p(so), p(rstd), M, N, EPS, s) == -1
    assert fwd(1, p(x), p(r), p(g), p(y), off(so), p(rstd), M, N, EPS, s) == -1
    bwd = lib.dl4j_rms_bwd
    assert lib.dl4j_rms_partial_rows(1100) == 128 and lib.dl4j_rms_partial_rows(5) == 5
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == 0
    assert bwd(1, p(y), p(x), p(g), p(rstd), p(r), p(r), p(part), p(dg), p(dsum), M, N, s) == 0   # dx aliases dres
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, 4104, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, 60, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, 0, N, s) == -1
    assert bwd(-1, p(y), p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, None, p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), None, p(g), p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), None, p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), p(g), None, None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, None, p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, p(so), None, p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, p(so), p(part), None, None, M, N, s) == -1
    assert bwd(1, off(y), p(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), off(x), p(g), p(rstd), None, p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), off(r), p(so), p(part), p(dg), None, M, N, s) == -1
    assert bwd(1, p(y), p(x), p(g), p(rstd), None, off(so), p(part), p(dg), None, M, N, s) == -1
    F_ = 16
    gu, dgu = torch.zeros(M, 2 * F_ + 8, dtype=torch.bfloat16, device=DEV).reshape(-1), \
        torch.zeros(M * (2 * F_ + 8), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(M * F_ + 8, dtype=torch.bfloat16, device=DEV)
    sf, sb = lib.dl4j_swiglu_fwd, lib.dl4j_swiglu_bwd
    assert sf(1, p(gu), p(out), M, F_, s) == 0
    assert sf(1, p(gu), p(out), M, 12, s) == -1                                          # F % 8
    assert sf(1, p(gu), p(out), 0, F_, s) == -1
    assert sf(4, p(gu), p(out), M, F_, s) == -1
    assert sf(1, None, p(out), M, F_, s) == -1 and sf(1, p(gu), None, M, F_, s) == -1
    assert sf(1, off(gu), p(out), M, F_, s) == -1 and sf(1, p(gu), off(out), M, F_, s) == -1
    assert sb(1, p(gu), p(out), p(dgu), M, F_, s) == 0
    assert sb(1, p(gu), p(out), p(dgu), M, 12, s) == -1
    assert sb(1, p(gu), p(out), p(gu), M, F_, s) == -1                                    # dgu aliases gu
    assert sb(1, None, p(out), p(dgu), M, F_, s) == -1 and sb(1, p(gu), None, p(dgu), M, F_, s) == -1
    assert sb(1, p(gu), p(out), None, M, F_, s) == -1
    assert sb(1, off(gu), p(out), p(dgu), M, F_, s) == -1 and sb(1, p(gu), off(out), p(dgu), M, F_, s) == -1
    assert sb(1, p(gu), p(out), off(dgu), M, F_, s) == -1
    torch.cuda.synchronize()
    # the wrappers hand the refusal on as None and leave the operands alone
    wide = torch.ones(2, 4104, dtype=torch.bfloat16, device=DEV)
    odd = torch.ones(2, 60, dtype=torch.bfloat16, device=DEV)
    keep = torch.full((2, 64), 3.0, dtype=torch.bfloat16, device=DEV)
    ok = torch.ones(2, 64, dtype=torch.bfloat16, device=DEV)
    for t in (wide, odd):
        n = t.shape[1]
        assert TN.rms_fwd(t, g[:n], EPS) is None and bool((t == 1).all())
        assert TN.rms_bwd(t, t, g[:n], rstd[:2]) is None and bool((t == 1).all())
    assert TN.rms_fwd(ok, g[:64], EPS, None, s_out=keep) is None and bool((keep == 3).all())      # s_out without r
    assert TN.rms_fwd(ok, g[:64], EPS, ok.float()) is None                                        # another dtype
    assert TN.rms_bwd(ok, ok, g[:64], rstd[:2], dres=keep[:, :32]) is None and bool((keep == 3).all())
    gate = torch.ones(2, 24, dtype=torch.bfloat16, device=DEV)                                    # F = 12
    assert TN.swiglu(gate) is None and TN.swiglu_bwd(gate, gate[:, :12].contiguous()) is None
    gate = torch.ones(2, 32, dtype=torch.bfloat16, device=DEV)
    assert TN.swiglu_bwd(gate, gate[:, :16].contiguous(), dgu=gate) is None and bool((gate == 1).all())
    assert TN.swiglu(gate[:, :16]) is None                                                        # not contiguous


# ------------------------------------------------------------------------------------------------ (b) rms_fwd
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_rms_fwd_against_the_fp64_formula(dt, N):
    """|out - ref| <= 1.01 u |ref| + tiny for every element: one rounding of the 16-bit type plus 1 % of it for the fp32
    arithmetic (a sum of at most 64 squares per lane and six shuffle steps, one rsqrt, two multiplies)."""
    u, tiny = U[dt], TINY[dt]
    gamma = _gamma(N)
    gd = gamma.to(DEV)
    worst = 0.0
    for M in (1, 5, 67):
        x, r = _rows(dt, M, N, 1), _rows(dt, M, N, 2)
        ref, rstd_ref = _rms64(x, gamma)
        got = TN.rms_fwd(x.to(DEV), gd, EPS)
        assert got is not None
        y, s, rstd = got
        ratio = ((y.cpu().double() - ref).abs() / (1.01 * u * ref.abs() + tiny)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (M, ratio)
        assert ((rstd.cpu().double() - rstd_ref[:, 0]).abs() / rstd_ref[:, 0]).max().item() < 1e-5, M
        # with a residual: the stored sum is (x + r) rounded, and y / rstd are those of the unfused sequence
        want_s = (x.float() + r.float()).to(dt)
        y1, _, rstd1 = TN.rms_fwd(want_s.to(DEV), gd, EPS)
        xd, rd = x.to(DEV), r.to(DEV)
        y2, s2, rstd2 = TN.rms_fwd(xd, gd, EPS, rd)
        assert torch.equal(_bits(xd), _bits(x)) and torch.equal(_bits(rd), _bits(r)), M
        assert torch.equal(_bits(s2), _bits(want_s)), (M, "s_out")
        assert torch.equal(_bits(y2), _bits(y1)) and torch.equal(_bits(rstd2), _bits(rstd1)), (M, "fused vs unfused")
        ref2, _ = _rms64(want_s, gamma)
        assert ((y2.cpu().double() - ref2).abs() / (1.01 * u * ref2.abs() + tiny)).max().item() <= 1.0, M
        # s_out aliasing x, then r
        for alias in ("x", "r"):
            xa, ra = x.to(DEV), r.to(DEV)
            y3, s3, rstd3 = TN.rms_fwd(xa, gd, EPS, ra, s_out=xa if alias == "x" else ra)
            assert s3 is (xa if alias == "x" else ra)
            assert torch.equal(_bits(s3), _bits(want_s)) and torch.equal(_bits(y3), _bits(y1)), (M, alias)
            assert torch.equal(_bits(rstd3), _bits(rstd1)), (M, alias)
    print(f"rms_fwd {dt} N={N}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ (c) rms_bwd
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_rms_bwd_against_fp64(dt, N):
    gamma = _gamma(N)
    gd = gamma.to(DEV)
    for M in (1, 67, 1100):                  # 1100: more rows than one pass of the 128-block grid at 8 waves a block
        s, dy, dres = _rows(dt, M, N, 3), _rows(dt, M, N, 4), _rows(dt, M, N, 5)
        _, rstd64 = _rms64(s, gamma)
        rstd = rstd64[:, 0].float().to(DEV)
        xhat = s.double() * rstd64
        dxh = dy.double() * gamma.double()
        dx_ref = rstd64 * (dxh - xhat * (dxh * xhat).mean(-1, keepdim=True))
        dg_ref = (dy.double() * xhat).sum(0)
        sd, dyd = s.to(DEV), dy.to(DEV)
        for with_res in (False, True):
            want = dx_ref + dres.double() if with_res else dx_ref
            for with_sum in (False, True):
                tag = (M, with_res, with_sum)
                dsum = torch.full((N,), float("nan"), device=DEV) if with_sum else None
                dgo = torch.full((N,), float("nan"), device=DEV)
                rd = dres.to(DEV) if with_res else None
                got = TN.rms_bwd(dyd, sd, gd, rstd, rd, dgamma_out=dgo, dsum_out=dsum)
                assert got is not None, tag
                dx, dg = got
                assert dg.data_ptr() == dgo.data_ptr()
                assert torch.isfinite(dx).all() and torch.isfinite(dg).all(), tag
                e_dx, e_dg = _err(dx, want), _err(dg, dg_ref)
                assert e_dx <= TOL and e_dg <= TOL, (tag, e_dx, e_dg)
                if with_sum:
                    e_ds = _err(dsum, want.sum(0))
                    assert e_ds <= TOL, (tag, e_ds)
                    cols = dx.float().cpu()
                    gap = (dsum.cpu() - cols.sum(0)).abs() - 1e-5 * cols.abs().sum(0)
                    assert gap.max().item() <= 0.0, (tag, "dsum is not the column sum of dx", gap.max().item())
                # two runs give the same bits
                dsum2 = torch.empty(N, device=DEV) if with_sum else None
                dx2, dg2 = TN.rms_bwd(dyd, sd, gd, rstd, rd, dsum_out=dsum2)
                assert torch.equal(_bits(dx2), _bits(dx)) and torch.equal(_bits(dg2), _bits(dg)), tag
                if with_sum:
                    assert torch.equal(_bits(dsum2), _bits(dsum)), tag
                if with_res:                 # dx written over dres
                    ra = dres.to(DEV)
                    dsum3 = torch.empty(N, device=DEV) if with_sum else None
                    dx3, dg3 = TN.rms_bwd(dyd, sd, gd, rstd, ra, dsum_out=dsum3, dx_out=ra)
                    assert dx3 is ra and torch.equal(_bits(dx3), _bits(dx)) and torch.equal(_bits(dg3), _bits(dg)), tag
                    if with_sum:
                        assert torch.equal(_bits(dsum3), _bits(dsum)), tag
        assert torch.equal(_bits(sd), _bits(s)) and torch.equal(_bits(dyd), _bits(dy)), M


# ------------------------------------------------------------------------------------------------ (d) swiglu
PLANTED = [0.0, 30.0, -30.0, 100.0, -100.0]


@functools.lru_cache(maxsize=None)
def _gate_up(dt, M, F_):
    """gu [M, 2F] = randn * 3 with the planted gates in the first columns of every row; df [M, F]. On the CPU."""
    g = torch.Generator().manual_seed(1000 * F_ + M)
    gu = torch.randn(M, 2 * F_, generator=g) * 3.0
    gu[:, :len(PLANTED)] = torch.tensor(PLANTED)
    return gu.to(dt), torch.randn(M, F_, generator=g).to(dt)


@pytest.mark.parametrize("F_", [8, 776, 2048])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_swiglu_forward_and_backward_against_fp64(dt, F_):
    """Forward: every element within one rounding, |out - ref| <= 1.01 u |ref| + tiny. Backward:
    |dg - ref| <= 1.01 u |ref| + 2^-20 |df u| (1 + |g|) + tiny: the middle term covers about sixteen fp32 roundings of
    terms no larger than that around the zero of silu' (g = -1.278), where the factor 1 + g (1 - sig) cancels. du has
    no cancelling factor and is held to the forward's bound."""
    u_, tiny = U[dt], TINY[dt]
    for M in (1, 67):
        gu, df = _gate_up(dt, M, F_)
        g, up, d = gu[:, :F_].double(), gu[:, F_:].double(), df.double()
        sig = 1.0 / (1.0 + torch.exp(-g))
        ref = g * sig * up
        gud = gu.to(DEV)
        out = TN.swiglu(gud)
        assert out is not None and out.shape == (M, F_) and out.dtype == dt
        assert torch.isfinite(out).all(), M
        ratio = ((out.cpu().double() - ref).abs() / (1.01 * u_ * ref.abs() + tiny)).max().item()
        assert ratio <= 1.0, (M, "forward", ratio)
        dg_ref = d * up * sig * (1.0 + g * (1.0 - sig))
        du_ref = d * g * sig
        dgu = TN.swiglu_bwd(gud, df.to(DEV))
        assert dgu is not None and dgu.shape == gu.shape and torch.isfinite(dgu).all(), M
        got = dgu.cpu().double()
        bound_g = 1.01 * u_ * dg_ref.abs() + 2.0 ** -20 * (d * up).abs() * (1.0 + g.abs()) + tiny
        r_g = ((got[:, :F_] - dg_ref).abs() / bound_g).max().item()
        r_u = ((got[:, F_:] - du_ref).abs() / (1.01 * u_ * du_ref.abs() + tiny)).max().item()
        assert r_g <= 1.0 and r_u <= 1.0, (M, "backward", r_g, r_u)
        assert torch.equal(_bits(gud), _bits(gu)), M
        # into a buffer of the caller's, bitwise the same
        mine = torch.empty_like(gud)
        assert TN.swiglu_bwd(gud, df.to(DEV), dgu=mine) is mine and torch.equal(_bits(mine), _bits(dgu)), M
        print(f"swiglu {dt} F={F_} M={M}: error / bound forward {ratio:.3f}, dg {r_g:.3f}, du {r_u:.3f}")


# ------------------------------------------------------------------------------------------------ (e) network
V = 77
LLAMA = dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu")


def _lm(dt, device, **kw):
    return TextGenerationTransformer(numLabels=V, hidden=256, layers=2, heads=4, nKVHeads=2, inputShape=[16],
                                     maxPositions=96, seed=5, dataType=dt, positionEncoding="rotary",
                                     **dict(LLAMA, **kw)).init(device=device)


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.to(dst.flattenedParams.device))
    dst._params_changed()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


NET_DTS = [DataType.BFLOAT16, DataType.HALF]


@pytest.mark.parametrize("dt", NET_DTS, ids=IDS)
def test_training_step_matches_fp32_cpu(dt):
    """The measure and bound of tests/test_gpu_rope.py for the same comparison: gradient rel L2 < 3e-2."""
    gpu, cpu = _lm(dt, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    assert "final_norm" in gpu.layers_by_name and "ln1b" not in gpu.layers_by_name["decoder_0"].params
    g = torch.Generator().manual_seed(3)
    T = 70
    x = torch.randint(0, V, (3, T), generator=g)
    y = torch.zeros(3, V, T)
    y.scatter_(1, torch.randint(0, V, (3, 1, T), generator=g), 1.0)
    fallback.reset()
    gpu.computeGradientAndScore([x.to(DEV)], [y.to(DEV)])
    torch.cuda.synchronize()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    assert fallback.count() == 0, fallback.summary()
    cpu.computeGradientAndScore([x], [y])
    ga, gb = gpu.flattenedGradients.float().cpu(), cpu.flattenedGradients.float()
    rel = float((ga - gb).norm() / gb.norm())
    print(f"llama training step {dt} GPU vs fp32 CPU: gradient rel {rel:.3e}, scores {gpu.score():.5f} "
          f"{cpu.score():.5f}")
    assert rel < 3e-2, rel
    assert abs(gpu.score() - cpu.score()) < 3e-2 * abs(cpu.score())


def _loop_greedy(net, prompt, n):
    """The loop a user writes on rnnTimeStep (tests/test_gpu_generation.py): argmax of the fp32 output, fed back."""
    net.rnnClearPreviousState()
    out = net.rnnTimeStep(prompt)[0]
    toks, dists = [], []
    for _ in range(n):
        p = out[:, :, -1]
        dists.append(p.float().cpu())
        t = p.argmax(1)
        toks.append(t)
        out = net.rnnTimeStep(t[:, None])[0]
    return torch.stack(toks, 1).cpu(), dists


@pytest.mark.parametrize("dt", NET_DTS, ids=IDS)
def test_generation_end_to_end(dt):
    N = 24
    gpu, cpu = _lm(dt, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    prompt = torch.randint(0, V, (3, 5), generator=torch.Generator().manual_seed(2))
    want, dists = _loop_greedy(gpu, prompt.to(DEV), N)
    fallback.reset()
    r = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert torch.equal(r.tokens.cpu(), want)
    # the fp32 CPU loop fed the same tokens: every step's distribution, compared as the layers are (rel L2 < 3e-2)
    cpu.rnnClearPreviousState()
    out = cpu.rnnTimeStep(prompt)[0]
    for i in range(N):
        assert _rel(dists[i], out[:, :, -1]) < 3e-2, i
        out = cpu.rnnTimeStep(want[:, i:i + 1])[0]
    pinned = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0, pinPositions=True)
    assert torch.equal(pinned.tokens, r.tokens)
    graph = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0, useGraph=True)
    stats = gpu.lastGenerationStats
    assert torch.equal(graph.tokens, pinned.tokens) and torch.equal(graph.scores, pinned.scores)
    assert stats["captures"] == 1 and stats["graphReplays"] > 0
    assert fallback.count() == 0, fallback.summary()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    # the fp8 cache: generation runs on the kernels too
    gpu.rnnClearPreviousState()
    gpu.rnnSetCacheDataType("fp8")
    r8 = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert r8.tokens.shape == r.tokens.shape and fallback.count() == 0, fallback.summary()
    assert gpu.rnnGetPreviousState("decoder_0")["kv"].shape == (3, 5 + N - 1, TN.kv_fp8_row_bytes(2, 64))


@pytest.mark.parametrize("dt", NET_DTS, ids=IDS)
def test_ragged_prompts_equal_every_row_alone(dt):
    net = _lm(dt, DEV)
    N, lens = 24, [5, 3]
    prompt = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(4)).to(DEV)
    fallback.reset()
    got = net.generate(prompt, promptLengths=lens, maxNewTokens=N)
    for b, n in enumerate(lens):
        alone = net.generate(prompt[b:b + 1, :n].contiguous(), maxNewTokens=N)
        assert torch.equal(got.tokens[b:b + 1], alone.tokens), f"row {b} ({n} tokens)"
    assert fallback.count() == 0, fallback.summary()


# the profiler method and the rule of tests/test_gpu_step_kernels.py
def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


def _profiled(step, warm=2):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        step()                                 # warm-up: autotuners / kernel-choice database, arena sizing
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_a_training_step_launches_no_torch_compute_kernels():
    net = _lm(DataType.BFLOAT16, DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V, (8, 64), generator=g).to(DEV)
    y = torch.zeros(8, V, 64)
    y.scatter_(1, torch.randint(0, V, (8, 1, 64), generator=g), 1.0)
    y = y.to(DEV)
    fallback.reset()
    names = _profiled(lambda: net.fit([x], [y]))
    assert len(names) > 20, names
    assert sum("rms_fwd_kernel" in n for n in names) == 5 and sum("rms_bwd_block" in n for n in names) == 5
    assert sum("swiglu_fwd_kernel" in n for n in names) == 2 and sum("swiglu_bwd_kernel" in n for n in names) == 2
    torch_ks = sorted({n for n in names if _is_torch_kernel(n)})
    assert not torch_ks, f"torch compute kernels in the training step: {torch_ks[:6]}"
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()


# as in tests/test_gpu_rope.py: rnnTimeStep ends with the fp32 conversion of the output layer's activations
_ALLOWED = ("bfloat16tofloat32_copy_kernel",)


def test_a_decode_step_launches_no_torch_compute_kernels():
    net = _lm(DataType.BFLOAT16, DEV)
    x = torch.randint(0, V, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    it = iter(steps)
    names = _profiled(lambda: net.rnnTimeStep(next(it)))
    assert len(names) > 10, names
    assert sum("rms_fwd_kernel" in n for n in names) == 5 and sum("swiglu_fwd_kernel" in n for n in names) == 2
    assert sum("rope_append" in n for n in names) == 2
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
