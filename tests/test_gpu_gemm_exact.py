"""The GEMM family on operands without rounding (tests/_exact_operands.py): every kernel's output must be the fp64
product rounded once to the output type, bit for bit. A dropped, duplicated or misplaced term, a neighbouring group's
scale byte, a partial plane skipped in a split-K merge or a second rounding in an epilogue changes bits; the tolerance
tests of the same kernels let all of these pass at some shapes. tests/test_exact_operands.py shows on the CPU that the
operands deserve the name and that planted errors move the expected bits at every shape used here.

(a) the skinny 16-bit product, (b) its grouped form, (c) the weight-quantised products, dense and grouped, (d) mmul's
tile configurations, layouts, types and epilogues, (e) the streaming kernel, (f) the grouped MFMA GEMM of the
mixture-of-experts block. GELU is not exact: the decode kernels' GELU epilogue is bounded against fp64 GELU of the
exact pre-activation by the output rounding plus the measured error of the device function (test_gelu_*)."""
import pytest
import torch

import _exact_operands as EO
from deeplearning4j_amd.ops import fallback, gemm
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTS = list(EO.DTS)
IDS = ["bf16", "fp16"]
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
X, TOPK = EO.X, EO.TOPK


def _same_bits(got, want, what):
    """got (any device) and want (CPU) hold the same bits; else the first differing element is reported."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype}"
    diff = EO.bits(got) != EO.bits(want)
    if diff.any():
        at = tuple(diff.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, the first at {at}: got "
                             f"{got[at].item()!r}, want {want[at].item()!r}")


def _framed(t, dt):
    """CPU [R, C] -> the same values on the GPU as a view of a NaN buffer whose row pitch is a multiple of 8 beyond C:
    a read past a row's end brings NaN."""
    R, C = t.shape
    buf = torch.full((R, (C + 7) // 8 * 8 + 8), NAN, dtype=dt, device=DEV)
    buf[:, :C] = t.to(dt).to(DEV)
    return buf[:, :C]


def _out_frame(rows, N, dt, aligned):
    """(buffer of NaN with 2 rows after ``rows`` and columns after N, its [rows, N] corner). aligned: a row pitch
    that is a multiple of 8 (vector stores); else N + 5 (element stores)."""
    buf = torch.full((rows + 2, (N + 7) // 8 * 8 + 8 if aligned else N + 5), NAN, dtype=dt, device=DEV)
    return buf, buf[:rows, :N]


def _epilogue(i):
    """(beta, bias in 16 bits) of the i-th launch: the four combinations in turn."""
    return float(i & 1), bool(i & 2)


def _dense_launch(call, x, w, bias, c0, dt, i, aligned, what):
    """One dense decode product out = x @ W + bias + beta * c0 in a NaN frame against the fp64 result rounded once."""
    M, N = x.shape[0], w.shape[1]
    beta, b16 = _epilogue(i)
    want = EO.expected(x @ w + bias + beta * c0, dt)
    buf, out = _out_frame(M, N, dt, aligned)
    if beta:
        out.copy_(c0.to(dt))
    fallback.reset()
    r = call(_framed(x, dt), (bias.to(dt) if b16 else bias.float()).to(DEV), out, beta)
    assert r is out and fallback.count() == 0, f"{what}: {fallback.summary()}"
    host = buf.cpu()
    assert host[M:].isnan().all() and host[:, N:].isnan().all(), f"{what}: something outside [M, N] changed"
    _same_bits(host[:M, :N], want, f"{what} beta={beta} bias16={b16} aligned={aligned}")


# ------------------------------------------------------------------------------------------------ (a) skinny, dense
def _skinny_weight(w, dt, layout):
    return _framed(w, dt) if layout == "n" else _framed(w.t(), dt).t()


def _skinny_case(dt, layout, width, M, K, N, i, split=False):
    x, w, bias, c0 = EO.dense(M, K, N)
    EO.assert_exact(x, w, bias.abs() + c0.abs(), dt)
    wg = _skinny_weight(w, dt, layout)
    if split:
        assert TN._lib().dl4j_skinny_gemm_workspace(width, M, N, K, wg.stride(0), wg.stride(1)) > 0, (M, K, N)
    for aligned in (False, True):
        _dense_launch(lambda xg, bg, out, beta: TN.skinny_gemm(xg, wg, bg, None, out, beta, width=width),
                      x, w, bias, c0, dt, i + aligned, aligned, f"skinny {layout}{width} {dt} M={M} K={K} N={N}")


LAYOUTS = [("n", 4), ("n", 8), ("k", 0)]
LAYOUT_IDS = ["n4", "n8", "k"]


@pytest.mark.parametrize("layout,width", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_skinny_gemm(dt, layout, width):
    """Every (M, K, N) of the lists on one layout: K and N tails of every kind, one to four row fragments, both store
    forms, both bias types, beta 0 and 1. K = 520 runs split (asserted), so the partial store and the merge launch see
    a K tail and masked columns."""
    i = 0
    for M in EO.SKINNY_M:
        for K in EO.SKINNY_K:
            for N in EO.SKINNY_N:
                _skinny_case(dt, layout, width, M, K, N, i, split=K == EO.SKINNY_SPLIT_K)
                i += 1


@pytest.mark.parametrize("M,K,N", EO.SKINNY_LONG, ids=lambda v: str(v))
def test_skinny_gemm_long_k(M, K, N):
    """The shapes at which the tolerance of tests/test_gpu_skinny_gemm.py lets a dropped k row pass."""
    for i, (layout, width) in enumerate(LAYOUTS):
        _skinny_case(BF16, layout, width, M, K, N, i)


# ---------------------------------------------------------------------------------------------- (b) skinny, grouped
def _grouped_case(launch, fmt, dt, K, N, Ntok, kind, gather, aligned, what):
    """One grouped decode product in a NaN frame: live rows bit-equal, nothing else written. ``launch(x, w, bias,
    plan, out)`` gets x framed on the GPU, the CPU weights [X, K, N], the fp32 bias and the plan on the GPU."""
    x, w, bias = EO.grouped(fmt, K, N, Ntok)
    p = EO.plan(kind, Ntok)
    a, live = EO.grouped_rows(p, x)
    for e in range(X):
        seg = slice(int(p.off[e]), int(p.off[e]) + int(p.cnt[e]))
        if p.cnt[e]:
            EO.assert_exact(a[seg], w[e], bias[e].abs().expand(int(p.cnt[e]), N), dt)
    want = EO.expected(EO.grouped_reference(p, a, w, bias), dt)
    xin = x if gather else torch.where(live.unsqueeze(1), a, torch.full_like(a, NAN))     # unowned rows hold NaN
    gpu_plan = p._replace(**{f: getattr(p, f).to(DEV) for f in ("cnt", "off", "src_of")})
    buf, out = _out_frame(p.rows, N, dt, aligned)
    fallback.reset()
    r = launch(_framed(xin, dt), w, bias.float().to(DEV), gpu_plan, out)
    what = f"{what} {dt} K={K} N={N} Ntok={Ntok} plan={kind} gather={gather} aligned={aligned}"
    assert r is out and fallback.count() == 0, f"{what}: {fallback.summary()}"
    host = buf.cpu()
    assert host[p.rows:].isnan().all() and host[:, N:].isnan().all(), f"{what}: something outside [Rcap, N] changed"
    assert host[:p.rows][~live].isnan().all(), f"{what}: a pad row or an idle expert's segment was written"
    _same_bits(host[:p.rows, :N][live], want[live], what)


def _stacked(w, dt):
    """[X, K, N] -> the N-contiguous stacked parameter as a view of a NaN buffer with a pitch beyond N."""
    Xn, K, N = w.shape
    flat = _framed(w.reshape(Xn * K, N), dt)
    return flat.as_strided((Xn, K, N), (K * flat.stride(0), flat.stride(0), 1))


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "sorted"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_skinny_gemm_grouped(dt, gather):
    """Both load widths, both plans (idle experts last; first and a middle one: the compact-row prefix and the
    merge's expert search walk cnt), every expert's matrix drawn on its own. (520, 136) runs split (asserted)."""
    lib = TN._lib()
    for width in (4, 8):
        for K, N in EO.GROUPED_KN:
            for i, Ntok in enumerate(EO.GROUPED_NTOK):
                if (K, N) == EO.GROUPED_SPLIT_KN:
                    assert lib.dl4j_skinny_gemm_grouped_workspace(width, Ntok, TOPK, X, N, K) > 0, (width, Ntok)
                for j, kind in enumerate(EO.PLANS):
                    _grouped_case(lambda xg, w, bg, pl, out: TN.skinny_gemm_grouped(
                        xg, _stacked(w, dt), bg, pl, gather, None, out, width=width),
                        None, dt, K, N, Ntok, kind, gather, bool((i + j) & 1), f"skinny grouped width {width}")


# ------------------------------------------------------------------------------------------------ (c) weight-quantised
def _quantised(w, fmt, dt, what):
    """dl4j_wq_quantize's QuantWeight of w on the GPU, after its bytes were found to be the reference's."""
    want = TN.wq_quantize_reference(w.to(dt), fmt)
    assert torch.equal(TN.wq_dequantize_reference(want, torch.float64), w), f"{what}: the weights are off the grid"
    got = TN.wq_quantize(w.to(dt).to(DEV), fmt)
    assert torch.equal(got.codes.cpu(), want.codes) and torch.equal(got.scales.cpu(), want.scales), what
    return got


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", EO.FMTS)
def test_wq_gemm(fmt, dt):
    """Grid weights: dequantisation is exact and the scale bytes differ between k groups and between columns. The
    format takes K % 32 == 0 only, so the deep shapes are (288, 40) and (544, 33). wq_split of csrc/gemm_wq.hip splits
    in chunks of 256 k and only while K * bits / (64 M) >= 2: K = 288 is the smallest K that splits (asserted through
    the workspace query, with K = 256 as the unsplit neighbour); the rule is mirrored here for every (M, K)."""
    lib, bits = TN._lib(), TN.WQ_FORMATS[fmt]
    assert lib.dl4j_wq_gemm_workspace(bits, 1, 40, 256) == 0 and lib.dl4j_wq_gemm_workspace(bits, 1, 40, 288) > 0
    for K, N in EO.WQ_REFUSED_KN:
        assert lib.dl4j_wq_gemm_workspace(bits, 1, N, K) == -1
    i = 0
    for K, N in EO.WQ_KN:
        for M in EO.SKINNY_M:
            x, w, bias, c0 = EO.mx(fmt, M, K, N)
            EO.assert_exact(x, w, bias.abs() + c0.abs(), dt)
            what = f"wq {fmt} {dt} M={M} K={K} N={N}"
            qw = _quantised(w, fmt, dt, what)
            split = K >= EO.WQ_SPLIT_K and K * bits // (64 * M) >= 2
            assert (lib.dl4j_wq_gemm_workspace(bits, M, N, K) > 0) == split, what
            _dense_launch(lambda xg, bg, out, beta: TN.wq_gemm(xg, qw, bg, None, out, beta),
                          x, w, bias, c0, dt, i, False, what)
            _dense_launch(lambda xg, bg, out, beta: TN.wq_linear(xg, qw, bg, None, out, beta),
                          x, w, bias, c0, dt, i + 1, True, what)
            i += 1


def _quantised_experts(w, fmt, dt, what):
    qs = [TN.wq_quantize_reference(w[e].to(dt), fmt) for e in range(X)]
    got = TN.wq_quantize_experts(w.to(dt).to(DEV), fmt)
    assert torch.equal(got.codes.cpu(), torch.stack([q.codes for q in qs])), what
    assert torch.equal(got.scales.cpu(), torch.stack([q.scales for q in qs])), what
    return got


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "sorted"])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", EO.FMTS)
def test_wq_gemm_grouped(fmt, dt, gather):
    """The grouped product on both plans; wq_split_grouped's rule (chunks of 256 k, active K bits / (64 A) >= 2 with
    A = Ntok * k assignments on min(X, A) active experts) is mirrored, and must split at one token from K = 288."""
    lib, bits = TN._lib(), TN.WQ_FORMATS[fmt]
    assert lib.dl4j_wq_gemm_grouped_workspace(bits, 1, TOPK, X, 40, 288) > 0
    for K, N in EO.WQ_KN:
        for i, Ntok in enumerate(EO.GROUPED_NTOK):
            A = Ntok * TOPK
            split = K >= EO.WQ_SPLIT_K and min(X, A) * K * bits // (64 * A) >= 2
            assert (lib.dl4j_wq_gemm_grouped_workspace(bits, Ntok, TOPK, X, N, K) > 0) == split, (K, N, Ntok)
            qe = _quantised_experts(EO.grouped(fmt, K, N, Ntok)[1], fmt, dt, f"experts {fmt} {dt} K={K} N={N}")
            for j, kind in enumerate(EO.PLANS):
                _grouped_case(lambda xg, w, bg, pl, out: TN.wq_gemm_grouped(xg, qe, bg, pl, gather, None, out),
                              fmt, dt, K, N, Ntok, kind, gather, bool((i + j) & 1), f"wq grouped {fmt}")


# ------------------------------------------------------------------------- one expert: the grouped product IS the dense
def _one_expert(Ntok, K, dt):
    """Random (not exact: another summation order would show) x [Ntok, K] and the expert-sorted buffer of the plan
    moe_route makes of [Ntok, 1] logits: (x, sorted x, plan, the live rows off[0] .. off[0] + Ntok - 1)."""
    x = (torch.randn(Ntok, K, generator=EO.gen("one expert x", Ntok, K)) * 0.5).to(dt).to(DEV)
    plan, _ = TN.moe_route(torch.zeros(Ntok, 1, device=DEV), 1)
    assert plan.cnt.cpu().tolist() == [Ntok]
    live = slice(int(plan.off[0]), int(plan.off[0]) + Ntok)
    xs = torch.full((plan.rows, K), NAN, dtype=dt, device=DEV)
    xs[live] = x[plan.src_of[live].long()]                                  # k = 1: the assignment is the token
    return x, xs, plan, live


ONE_EXPERT = {"skinny": ((3, 96, 77, False), (17, 96, 77, False), (64, 96, 77, False), (3, 3072, 80, True)),
              "wq": ((3, 96, 77, False), (17, 96, 77, False), (64, 96, 77, False), (3, 288, 40, True))}


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("family,how", [("skinny", 4), ("skinny", 8), ("wq", "fp8"), ("wq", "fp4")],
                         ids=["width4", "width8", "fp8", "fp4"])
def test_grouped_of_one_expert_is_the_dense_product(family, how, dt):
    """X = 1, k = 1, a sorted plan, an fp32 bias, no activation: the live rows of skinny_gemm_grouped / wq_gemm_grouped
    are the rows of skinny_gemm / wq_gemm on the same weight bytes, bit for bit: one block body, one epilogue, one
    merge and one split rule per family. The dense and the grouped workspace queries agree at every case, so the two
    run the same geometry; the last case of each family splits K (asserted)."""
    lib = TN._lib()
    for Ntok, K, N, split in ONE_EXPERT[family]:
        g = EO.gen("one expert", family, how, Ntok, K, N)
        w = torch.randn(K, N, generator=g) * 0.1
        bias = torch.randn(N, generator=g).to(DEV)
        x, xs, plan, live = _one_expert(Ntok, K, dt)
        if family == "skinny":
            wg = _framed(w, dt)
            sizes = (lib.dl4j_skinny_gemm_workspace(how, Ntok, N, K, wg.stride(0), wg.stride(1)),
                     lib.dl4j_skinny_gemm_grouped_workspace(how, Ntok, 1, 1, N, K))
            dense = lambda: TN.skinny_gemm(x, wg, bias, None, width=how)  # noqa: E731
            grouped = lambda: TN.skinny_gemm_grouped(xs, wg.unsqueeze(0), bias, plan, False, width=how)  # noqa: E731
        else:
            bits, qw = TN.WQ_FORMATS[how], TN.wq_quantize(w.to(dt).to(DEV), how)
            qe = TN.QuantExperts(how, 1, K, N, qw.codes.unsqueeze(0), qw.scales.unsqueeze(0))
            sizes = (lib.dl4j_wq_gemm_workspace(bits, Ntok, N, K),
                     lib.dl4j_wq_gemm_grouped_workspace(bits, Ntok, 1, 1, N, K))
            dense = lambda: TN.wq_gemm(x, qw, bias)  # noqa: E731
            grouped = lambda: TN.wq_gemm_grouped(xs, qe, bias, plan, False)  # noqa: E731
        what = f"{family} {how} {dt} Ntok={Ntok} K={K} N={N}"
        assert sizes[0] == sizes[1] and (sizes[0] > 0) == split, f"{what}: workspaces {sizes}"
        fallback.reset()
        d, r = dense(), grouped()
        assert d is not None and r is not None and fallback.count() == 0, f"{what}: {fallback.summary()}"
        _same_bits(r[live], d.cpu(), what)


# ------------------------------------------------------------------------------------------------ GELU epilogues
# max |gelu_f(z) - GELU(z)| of csrc/mfma_tile.h's device function over fp32 z in [-8, 8], measured on MI355X by
# _device_gelu_error below against fp64 GELU of the same fp32 inputs: GELU_F_MEASURED. The tests allow twice that.
GELU_F_MEASURED = 4.6e-07
# half an ulp of a value in [2^(e-1), 2^e): 2^-9 (bf16, 8 significant bits) / 2^-12 (fp16, 11) times 2^e
HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}


def _gelu64(z):
    return torch.nn.functional.gelu(z.double())


def _device_gelu_error():
    """The device GELU alone: the fp32 product I @ Z (exact, checked) through mmul's GELU epilogue, fp32 out, against
    fp64 GELU of the same fp32 z: a dense sweep of [-8, 8] and the multiples of 2^-6 the exact cases can produce."""
    n = 256
    z = torch.cat([torch.linspace(-8, 8, n * (n - 8), dtype=torch.float64).float(),
                   (torch.arange(-8 * 64, 8 * 64 + 1) / 64.0).float(), torch.zeros(8 * n - 1025)]).reshape(n, n)
    eye = torch.eye(n, device=DEV)
    assert torch.equal(gemm.mmul(eye, z.to(DEV)).cpu(), z), "the fp32 product by the identity is exact"
    got = gemm.mmul(eye, z.to(DEV), act="gelu").cpu()
    return (got.double() - _gelu64(z)).abs().max().item()


def _gelu_check(got, z64, dt, what):
    """|got - GELU(z)| <= half an ulp of the output type at the fp32 value that is rounded (HALF_ULP times the power
    of two above it; fp16 subnormals: of 2^-14) + twice the measured error of the device function."""
    e2 = 2 * GELU_F_MEASURED
    g = _gelu64(z64)
    top = torch.exp2(torch.frexp(g.abs() + e2).exponent.double())
    if dt == torch.float16:
        top = top.clamp_min(2.0 ** -13)
    bound = HALF_ULP[dt] * top + e2
    err = (got.cpu().double() - g).abs()
    worst = (err - bound).max().item()
    print(f"{what}: device gelu_f error now {_device_gelu_error():.3e} (recorded {GELU_F_MEASURED:.3e}), max err "
          f"{err.max().item():.3e}, closest to its bound by {-worst:.3e}")
    assert worst <= 0, f"{what}: {int((err > bound).sum())} elements beyond the bound, worst by {worst:.3e}"


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_gelu_skinny_gemm(dt):
    """GELU of an exact pre-activation in |z| <= 8 on the three layouts, unsplit (40, 24) and split (520, 77).
    Measured on MI355X: max |gelu_f - GELU| = 4.6e-7 over fp32 z in [-8, 8] (GELU_F_MEASURED). Bound per element:
    half an ulp of the output (2^-9 bf16 / 2^-12 fp16 times the power of two above the value) + 2 * 4.6e-7."""
    for M, K, N in ((17, 40, 24), (5, 520, 77)):
        x, w, bias, _ = EO.dense(M, K, N)
        w, bias = EO.gelu_scaled(x, w, bias)
        EO.assert_exact(x, w, bias.abs().expand(M, N), dt)
        for layout, width in LAYOUTS:
            buf, out = _out_frame(M, N, dt, False)
            fallback.reset()
            r = TN.skinny_gemm(_framed(x, dt), _skinny_weight(w, dt, layout), bias.float().to(DEV), "gelu", out,
                               width=width)
            assert r is out and fallback.count() == 0, fallback.summary()
            _gelu_check(out, x @ w + bias, dt, f"gelu skinny {layout}{width} {dt} M={M} K={K} N={N}")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", EO.FMTS)
def test_gelu_wq_gemm(fmt, dt):
    """As test_gelu_skinny_gemm on the quantised product, unsplit (96, 77) and split (544, 33); same bound."""
    for M, K, N in ((17, 96, 77), (5, 544, 33)):
        x, w, bias, _ = EO.mx(fmt, M, K, N)
        w, bias = EO.gelu_scaled(x, w, bias)
        EO.assert_exact(x, w, bias.abs().expand(M, N), dt)
        qw = _quantised(w, fmt, dt, f"gelu wq {fmt}")
        fallback.reset()
        out = TN.wq_gemm(_framed(x, dt), qw, bias.float().to(DEV), "gelu")
        assert out is not None and fallback.count() == 0, fallback.summary()
        _gelu_check(out, x @ w + bias, dt, f"gelu wq {fmt} {dt} M={M} K={K} N={N}")


def _gelu_grouped(launch, fmt, dt, K, N, Ntok, what):
    x, w, bias = EO.grouped(fmt, K, N, Ntok)
    p = EO.plan("first_and_middle_idle", Ntok)
    a, live = EO.grouped_rows(p, x)
    for e in (1, 3):                                                    # the two live experts, each scaled on its own
        w_e, b_e = EO.gelu_scaled(x, w[e], bias[e])
        w, bias = w.clone(), bias.clone()
        w[e], bias[e] = w_e, b_e
        EO.assert_exact(x, w[e], bias[e].abs().expand(Ntok, N), dt)
    z = EO.grouped_reference(p, a, w, bias)
    gpu_plan = p._replace(**{f: getattr(p, f).to(DEV) for f in ("cnt", "off", "src_of")})
    fallback.reset()
    out = launch(_framed(x, dt), w, bias.float().to(DEV), gpu_plan)
    assert out is not None and fallback.count() == 0, fallback.summary()
    _gelu_check(out.cpu()[live], z[live], dt, f"{what} {dt} K={K} N={N} Ntok={Ntok}")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_gelu_skinny_gemm_grouped(dt):
    """As test_gelu_skinny_gemm on the gathered grouped product (the W1 of an expert block); same bound."""
    for K, N in ((40, 24), (520, 136)):
        _gelu_grouped(lambda xg, w, bg, pl: TN.skinny_gemm_grouped(xg, _stacked(w, dt), bg, pl, True, "gelu"),
                      None, dt, K, N, 17, "gelu skinny grouped")


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", EO.FMTS)
def test_gelu_wq_gemm_grouped(fmt, dt):
    """As test_gelu_skinny_gemm on the gathered quantised grouped product; same bound."""
    for K, N in ((96, 77), (544, 33)):
        _gelu_grouped(lambda xg, w, bg, pl: TN.wq_gemm_grouped(
            xg, _quantised_experts(w, fmt, dt, "gelu experts"), bg, pl, True, "gelu"),
            fmt, dt, K, N, 17, f"gelu wq grouped {fmt}")


# ------------------------------------------------------------------------------------------------ (d) mmul
def _mk(t, dt, contig_last=True):
    """CPU [R, C] on the GPU in ``dt``; contig_last False: the transposed-view layout."""
    return t.to(dt).to(DEV) if contig_last else t.t().contiguous().to(dt).to(DEV).t()


@pytest.mark.parametrize("cfg", EO.MMUL_CFGS, ids=lambda c: f"cfg{c[0]}x{c[1]}")
def test_mmul_every_tile_config(cfg, monkeypatch):
    """Every kernel configuration (the split-K ones included) on the four operand layouts, M / N tails and a K tail,
    bf16 operands, fp32 and bf16 output."""
    monkeypatch.setattr(gemm, "_FORCE_CFG", cfg)
    for M, N, K in EO.MMUL_SHAPES:
        x, w, _, _ = EO.dense(M, K, N)
        EO.assert_exact(x, w, None, (BF16, F32))
        ref = x @ w
        for a_kc in (True, False):
            for b_kc in (True, False):
                a, b = _mk(x, BF16, a_kc), _mk(w, BF16, not b_kc)
                for odt in (F32, BF16):
                    fallback.reset()
                    out = gemm.mmul(a, b, out_dtype=odt)
                    assert fallback.count() == 0, fallback.summary()
                    _same_bits(out, EO.expected(ref, odt), f"mmul cfg {cfg} {M}x{N}x{K} a_kc={a_kc} b_kc={b_kc} {odt}")


@pytest.mark.parametrize("M,N,K", EO.MMUL_SHAPES + EO.MMUL_ODD, ids=lambda v: str(v))
def test_mmul_default_chooser(M, N, K):
    """The chooser's own pick: fp16 and bf16 operands into 16-bit and fp32 outputs, and the odd shapes that take the
    padded-copy / generic path."""
    x, w, _, _ = EO.dense(M, K, N)
    ref = x @ w
    for dt in DTS:
        EO.assert_exact(x, w, None, (dt, F32))
        for odt in (dt, F32):
            fallback.reset()
            out = gemm.mmul(_mk(x, dt), _mk(w, dt), out_dtype=odt)
            assert fallback.count() == 0, fallback.summary()
            _same_bits(out, EO.expected(ref, odt), f"mmul {dt}->{odt} {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", EO.MMUL_SHAPES, ids=lambda v: str(v))
def test_mmul_fp32_operands(M, N, K):
    """Integers up to 64 in fp32 on the in-tree fp32 path (no library candidate: nothing is counted as a fallback)."""
    x, w, _, _ = EO.dense(M, K, N, 64, 64)
    EO.assert_exact(x, w, None, F32)
    fallback.reset()
    out = gemm.mmul(_mk(x, F32), _mk(w, F32))
    assert fallback.count() == 0, fallback.summary()
    _same_bits(out, EO.expected(x @ w, F32), f"mmul fp32 {M}x{N}x{K}")
    out = gemm.mmul(_mk(x, F32, False), _mk(w, F32, False))
    _same_bits(out, EO.expected(x @ w, F32), f"mmul fp32 transposed views {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", EO.MMUL_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("odt", [F32, BF16], ids=["fp32out", "bf16out"])
def test_mmul_epilogues(odt, M, N, K):
    """alpha = 0.5 with beta = 1 and a row bias; a column-major destination; a 3-D batch of 3."""
    x, w, _, c0 = EO.dense(M, K, N)
    rb = EO.ints((M,), 1, 8, EO.gen("row bias", M))
    EO.assert_exact(0.5 * x, w, rb.abs().unsqueeze(1) + c0.abs(), (BF16, odt))
    a, b = _mk(x, BF16), _mk(w, BF16, False)
    out = c0.to(odt).to(DEV)
    fallback.reset()
    gemm.mmul(a, b, out=out, bias=rb.float().to(DEV), bias_dim=0, alpha=0.5, beta=1.0)
    _same_bits(out, EO.expected(0.5 * (x @ w) + rb.unsqueeze(1) + c0, odt), f"alpha / beta / row bias {odt}")
    view = torch.full((N * M,), NAN, dtype=odt, device=DEV).view(N, M).t()                # column-major [M, N]
    gemm.mmul(a, b, out=view)
    _same_bits(view, EO.expected(x @ w, odt), f"column-major destination {odt}")
    x3 = torch.stack([x, x.flip(0), x.roll(1, 0)])
    w3 = torch.stack([w, w.flip(1), w.roll(1, 1)])
    out = gemm.mmul(x3.to(BF16).to(DEV), w3.to(BF16).to(DEV), out_dtype=odt)
    _same_bits(out, EO.expected(x3 @ w3, odt), f"batch of 3 {odt}")
    assert fallback.count() == 0, fallback.summary()


@pytest.mark.parametrize("odt", [F32, BF16], ids=["fp32out", "bf16out"])
def test_mmul_forced_split_k_reduce(odt, monkeypatch):
    """The split-K reduce launch (configuration 3 in 3 splits, ragged tiles) with a column bias and beta = 1."""
    M, N, K = EO.MMUL_SHAPES[0]
    x, w, bias, c0 = EO.dense(M, K, N)
    EO.assert_exact(x, w, bias.abs() + c0.abs(), (BF16, odt))
    monkeypatch.setattr(gemm, "_FORCE_CFG", (3, 3))
    out = c0.to(odt).to(DEV)
    fallback.reset()
    gemm.mmul(_mk(x, BF16), _mk(w, BF16, False), out=out, bias=bias.float().to(DEV), beta=1.0)
    assert fallback.count() == 0, fallback.summary()
    _same_bits(out, EO.expected(x @ w + bias + c0, odt), f"split-K reduce {odt}")


# ------------------------------------------------------------------------------------------------ (e) streaming kernel
@pytest.mark.parametrize("N,K", EO.STREAM_NK)
def test_gemm_stream(N, K, monkeypatch):
    """Every (BN, K / 64, slots) variant at 40 m-tiles, bf16 and fp16, bias + ReLU: ReLU of an exact value is exact."""
    M = EO.STREAM_M
    x, w, bias, _ = EO.dense(M, K, N)
    monkeypatch.setattr(gemm, "_FORCE_CFG", gemm.STREAM_CFG)
    want64 = (x @ w + bias).clamp_min(0)
    for dt in DTS:
        EO.assert_exact(x, w, bias.abs().expand(M, N), dt)
        fallback.reset()
        out = gemm.mmul(_mk(x, dt), _mk(w, dt, False), bias=bias.float().to(DEV), act="relu", out_dtype=dt)
        assert fallback.count() == 0, fallback.summary()
        _same_bits(out, EO.expected(want64, dt), f"stream {dt} N={N} K={K}")


# ------------------------------------------------------------------------------------------------ (f) grouped MFMA GEMM
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("bkc", [False, True], ids=["Ncontig", "Kcontig"])
def test_gemm_grouped(dt, bkc):
    """tests/test_gpu_moe.py's (K, N) grid on its planted plan (an idle expert, a full tile, a one-row segment, a
    segment one row into its second tile): live rows bit-equal, dead tiles untouched."""
    plan, _ = TN.moe_route(EO.moe_planted_logits().to(DEV), TOPK)
    assert plan.cnt.cpu().tolist() == [0, EO.MOE_G, 1, EO.MOE_G + 1]
    src = plan.src_of.cpu().long()
    live = src >= 0
    rex = plan.tile_expert.cpu().long().repeat_interleave(EO.MOE_G)
    for K, N in EO.MOE_KN:
        x, w, bias = EO.moe(K, N)
        for e in range(X):
            EO.assert_exact(x, w[e], bias[e].abs().expand(x.shape[0], N), dt)
        xp = TN.moe_gather(x.to(dt).to(DEV), plan)
        a = x[src.clamp_min(0) // TOPK]
        ref = torch.zeros(plan.rows, N, dtype=torch.float64)
        for e in range(X):
            rows = live & (rex == e)
            ref[rows] = a[rows] @ w[e] + bias[e]
        wd = w.transpose(1, 2).contiguous().to(dt).to(DEV).transpose(1, 2) if bkc else w.to(dt).to(DEV)
        c = torch.full((plan.rows, N), NAN, dtype=dt, device=DEV)
        fallback.reset()
        assert TN.gemm_grouped(xp, wd, bias.float().to(DEV), plan, out=c) is c and fallback.count() == 0
        host = c.cpu()
        assert host[rex < 0].isnan().all(), "a dead tile was written"
        _same_bits(host[live], EO.expected(ref, dt)[live], f"grouped gemm {dt} K={K} N={N} bkc={bkc}")
