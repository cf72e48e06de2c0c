"""The reduction tail of bn_bwd_partial (csrc/batchnorm.hip bn_bwd_tail): on layers without a residual and with
C <= 512 the blocks of the partial pass fold their own partial rows (groups of G = 128 blocks, then one top-level fold
in double) and write dbeta / dgamma and the means, so no kernel runs between the partial pass and the apply pass. The
residual layers (res, rbn), wider rows, the forward statistics and the BN + ReLU + max-pool backward keep their
separate fold launches; they are covered here too, on the same shapes.

Reference and tolerances are those of tests/test_gpu_kernels.py::test_batchnorm_fwd_bwd: ops.bn_forward /
ops.bn_backward on CPU fp32 inputs (the "REF" context), dx within 2*tol (tol = 2e-2 bf16, 1e-4 fp32), dgamma / dbeta
within 3e-2 (bf16) / 1e-3 (fp32). fp16 carries 3 more mantissa bits than bf16, so its bounds are the bf16 ones / 8.

Shapes are chosen by the block count bn_bwd_grid (csrc/batchnorm.hip) makes of them: nb = floor(M*(C/8)/8192), rounded
up to a multiple of 256 from 256 on, capped at 2048, then re-derived from the rows per block:
    (16, 24)       1 block     no ticket at all
    (5000, 64)     4 blocks    one partial group
    (33809, 64)    33 blocks   one partial group; more than one of the fold launch's 32-row units
    (20000, 200)   61 blocks   C not a multiple of 64: channel guards in the tail's fourth 64-channel trip
    (130048, 64)   127 blocks  G - 1
    (131072, 64)   128 blocks  G: exactly one full group, still no top level
    (132096, 64)   129 blocks  G + 1: a full group and a group of one, the top level sums two folded rows
    (4096, 2048)   128 blocks  256 channel groups, one row per block iteration; too wide for the tail: fold launch
    (307200, 64)   512 blocks  block count rounded to a multiple of 256; four groups
    (25000, 512)   194 blocks  the widest rows the tail takes: eight 64-channel trips per group-folder"""
import functools

import pytest
import torch

from deeplearning4j_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(16, 24), (5000, 64), (33809, 64), (20000, 200), (130048, 64), (131072, 64), (132096, 64), (4096, 2048),
          (307200, 64), (25000, 512)]
TOL = {torch.bfloat16: 2e-2, torch.float16: 2e-2 / 8, torch.float32: 1e-4}
GTOL = {torch.bfloat16: 3e-2, torch.float16: 3e-2 / 8, torch.float32: 1e-3}
DECAY, EPS = 0.9, 1e-5


def _close(a, b, tol):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, f"max abs err {err} (scale {scale})"


def _expected_blocks(M, C):
    """bn_bwd_grid of csrc/batchnorm.hip."""
    nb = M * (C // 8) // 8192
    if nb >= 256:
        nb = (nb + 255) // 256 * 256
    nb = min(max(nb, 1), 2048)
    rpb = (M + nb - 1) // nb
    return (M + rpb - 1) // rpb


def test_shapes_give_the_block_counts_the_cases_are_named_for():
    assert [_expected_blocks(*s) for s in SHAPES] == [1, 4, 33, 61, 127, 128, 129, 128, 512, 194]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, variant):
    """Inputs (rounded to dtype) and the CPU fp32 reference of one case, computed once. variant: plain / relu /
    res (residual with ReLU mask) / rbn (residual that is the raw input of a folded-in shortcut BN)."""
    M, C = shape
    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 3 + 1.5).to(dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g).to(dtype)
    xr = (torch.randn(M, C, generator=g) * 0.7 - 0.3).to(dtype)
    gamma2 = torch.rand(C, generator=g) + 0.5
    beta2 = torch.randn(C, generator=g) * 0.1
    rm, rv, rm2, rv2 = torch.zeros(C), torch.ones(C), torch.zeros(C), torch.ones(C)
    ref = {}
    res = None
    if variant == "res":
        res = xr.float()
    elif variant == "rbn":
        res, rctx = ops.bn_forward(xr.float(), gamma2, beta2, rm2, rv2, True, DECAY, EPS)
    relu = variant != "plain"
    for _ in range(4):
        rm, rv = torch.zeros(C), torch.ones(C)
        y, ctx = ops.bn_forward(x.float(), gamma, beta, rm, rv, True, DECAY, EPS, relu, residual=res)
        assert ctx[0] == "REF"
        if not relu:
            break
        # Where the pre-activation sits within rounding noise of zero (fp32 noise here is ~1e-6) the ReLU mask of the
        # reference itself is arbitrary, and one such element among millions decides a whole dy of error: move those
        # inputs away (a quarter unit of x, far above the noise) and take the reference again.
        _, _, mean, invstd, gg, bb = ctx[:6]
        t = (x.float() - mean) * invstd * gg + bb + (res if res is not None else 0.0)
        ill = t.abs() < 1e-4
        if not ill.any():
            break
        x = torch.where(ill, (x.float() + 0.25).to(dtype), x)
    else:
        raise AssertionError("could not move the inputs off the ReLU threshold")
    dx, dg, db, dres = ops.bn_backward(dy.float(), ctx)
    ref.update(y=y, rm=rm, rv=rv, dx=dx, dg=dg, db=db, dres=dres)
    if variant == "rbn":
        dxr, dg2, db2, _ = ops.bn_backward(dres, rctx)
        ref.update(dres=dxr, dg2=dg2, db2=db2, rm2=rm2, rv2=rv2)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, xr=xr, gamma2=gamma2, beta2=beta2), ref


def _run(inp, variant, cuda):
    """The same case through the HIP kernels on the current stream."""
    C = inp["x"].shape[1]
    d = {k: v.to(cuda) for k, v in inp.items()}
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    out = {}
    res = rctx = rg = None
    if variant == "res":
        res = d["xr"]
    elif variant == "rbn":
        rm2, rv2 = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        r = ops.bn_forward(d["xr"], d["gamma2"], d["beta2"], rm2, rv2, True, DECAY, EPS, stats_only=True)
        assert r is not None and r[1][0] == "NATIVE_STATS"
        res, rctx = d["xr"], r[1][2]
        rg = (torch.empty(C, device=cuda), torch.empty(C, device=cuda))
        out.update(rm2=rm2, rv2=rv2)
    y, ctx = ops.bn_forward(d["x"], d["gamma"], d["beta"], rm, rv, True, DECAY, EPS, variant != "plain", residual=res,
                            rctx=rctx)
    assert ctx[0] == "NATIVE"
    dx, dg, db, dres = ops.bn_backward(d["dy"], ctx, rgrads=rg)
    out.update(y=y, rm=rm, rv=rv, dx=dx, dg=dg, db=db, dres=dres)
    if rg is not None:
        out.update(dg2=rg[0], db2=rg[1])
    return out


def _check(out, ref, dtype):
    tol, gtol = TOL[dtype], GTOL[dtype]
    _close(out["y"], ref["y"], tol)
    _close(out["rm"], ref["rm"], 1e-4)
    _close(out["rv"], ref["rv"], 1e-4)
    _close(out["dx"], ref["dx"], 2 * tol)
    _close(out["dg"], ref["dg"], gtol)
    _close(out["db"], ref["db"], gtol)
    if ref["dres"] is not None:
        _close(out["dres"], ref["dres"], 2 * tol)
    for k in ("dg2", "db2"):
        if k in ref:
            _close(out[k], ref[k], gtol)
    for k in ("rm2", "rv2"):
        if k in ref:
            _close(out[k], ref[k], 1e-4)


@pytest.mark.parametrize("shape", SHAPES)
def test_tail_matches_reference_bf16(cuda, shape):
    """Every block count, plain BN: y and the running statistics, dx / dgamma / dbeta (bn_bwd_partial's tail)."""
    inp, ref = _case(shape, torch.bfloat16, "plain")
    _check(_run(inp, "plain", cuda), ref, torch.bfloat16)


@pytest.mark.parametrize("variant", ["relu", "res", "rbn"])
@pytest.mark.parametrize("shape", [(33809, 64), (20000, 200), (132096, 64)])
def test_tail_variants_bf16(cuda, shape, variant):
    """The other bn_bwd_partial instantiations: relu ends in the tail, res and rbn in the fold launches (rbn: both
    layers' dgamma / dbeta and the gradient w.r.t. the shortcut BN's input)."""
    inp, ref = _case(shape, torch.bfloat16, variant)
    _check(_run(inp, variant, cuda), ref, torch.bfloat16)


@pytest.mark.parametrize("shape,dtype", [((33809, 64), torch.float32), ((20000, 200), torch.float32),
                                         ((5000, 64), torch.float16), ((33809, 64), torch.float16)])
@pytest.mark.parametrize("variant", ["plain", "relu", "res"])
def test_tail_other_dtypes(cuda, shape, dtype, variant):
    inp, ref = _case(shape, dtype, variant)
    _check(_run(inp, variant, cuda), ref, dtype)


def test_tail_4d_nhwc(cuda):
    """The (33809, 64) residual case as an NHWC 4-D tensor: 33809 = 1 x 1 x 33809 rows."""
    inp, ref = _case((33809, 64), torch.bfloat16, "res")
    to4 = lambda t: t.t().reshape(1, 64, 1, -1).contiguous(memory_format=torch.channels_last)  # noqa: E731
    inp4 = {k: (to4(v) if v.dim() == 2 else v) for k, v in inp.items()}
    out = _run(inp4, "res", cuda)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 64) if t is not None and t.dim() == 4 else t  # noqa: E731
    _check({k: rows(v) for k, v in out.items()}, ref, torch.bfloat16)


def test_bn_pool_tail_matches_composed_reference(cuda):
    """BN + ReLU + max pool 3x3/2 (unchanged kernels, kept as a guard): 8 x 64 x 64 pooled rows -> 42 blocks of
    bnpool_bwd_partial; the full pass over the 8 x 130 x 130 input rows runs bn_stats_partial with 176 blocks."""
    g = torch.Generator().manual_seed(7)
    C = 64
    x = (torch.randn(8, C, 130, 130, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    args = (True, DECAY, EPS, (3, 3), (2, 2), (0, 0, 0, 0))
    rm_c, rv_c = torch.zeros(C), torch.ones(C)
    y_ref, ctx_ref = ops.bn_pool_forward(x.float(), gamma, beta, rm_c, rv_c, *args)
    assert ctx_ref[0] == "COMPOSED"
    dy = torch.randn(y_ref.shape, generator=g).to(torch.bfloat16)
    dx_ref, dg_ref, db_ref = ops.bn_pool_backward(dy.float(), ctx_ref)
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    xd = x.to(cuda).contiguous(memory_format=torch.channels_last)
    y, ctx = ops.bn_pool_forward(xd, gamma.to(cuda), beta.to(cuda), rm, rv, *args)
    assert ctx[0] == "NATIVE_POOL"
    dx, dg, db = ops.bn_pool_backward(dy.to(cuda).contiguous(memory_format=torch.channels_last), ctx)
    tol = TOL[torch.bfloat16]
    _close(y, y_ref, tol)
    _close(rm, rm_c, 1e-4)
    _close(rv, rv_c, 1e-4)
    _close(dx, dx_ref, 2 * tol)
    _close(dg, dg_ref, GTOL[torch.bfloat16])
    _close(db, db_ref, GTOL[torch.bfloat16])


_KEYS = ("y", "dx", "dg", "db")


def test_tail_is_bitwise_reproducible_and_reuses_ticket_slots(cuda):
    """300 launches of the tail (two groups and a top level) wrap the pool of 256 ticket slots: the last arrivers
    reset their counters, so every run equals the first bitwise."""
    inp, _ = _case((132096, 64), torch.bfloat16, "relu")
    first = None
    for _ in range(300):
        out = _run(inp, "relu", cuda)
        if first is None:
            first = {k: out[k].clone() for k in _KEYS}
        else:
            for k in _KEYS:
                assert torch.equal(first[k], out[k]), k


def test_tail_on_two_streams(cuda):
    """The same case issued alternately on two streams of one device: launches in flight together hold different
    ticket slots, and both streams' outputs equal the single-stream result bitwise."""
    inp, _ = _case((132096, 64), torch.bfloat16, "relu")
    single = _run(inp, "relu", cuda)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    outs = []
    for i in range(16):
        with torch.cuda.stream(streams[i % 2]):
            outs.append(_run(inp, "relu", cuda))
    torch.cuda.synchronize()
    for out in outs:
        for k in _KEYS:
            assert torch.equal(single[k], out[k]), k
