"""The mixture-of-experts kernels (csrc/moe.hip, the grouped modes of csrc/gemm.hip) and the sparse block on the GPU,
bf16 and fp16.

(a) the refusals of every entry point; (b) the router and its plan, exactly the torch twin's on the same fp32 logits,
with a planted routing that gives an empty expert, an exactly full tile, a one-row segment and a segment one row into
its second tile; (c) the grouped GEMM against fp64 per live row, both B layouts, ragged K and N, dead tiles untouched,
the bits of a row independent of the other rows; (d) NaN in every pad row and dead tile changes no output bit; (e) the
grouped weight gradient and the segment sums against fp64; (f) combine, its backward and the router's backward; (g) a
two-block rotary rms / pre / swiglu language model with four experts against fp32 on the CPU.

The constants (unit roundoff ``U``, ``_err``, ``_bits``) are those of tests/test_gpu_rope.py, ``_tol`` is that of
tests/test_gpu_gemm.py.

MARGIN (g): the GPU and the fp32 CPU reference can only be asked for the same routing where no decision is a near-tie
that 16-bit rounding moves. Measured on the reference alone (tools/bench_moe.py --margin, the torch path on the GPU
with DL4J_AMD_NATIVE=0, since the CPU path computes the 16-bit types in fp32): the largest difference between the
router logits of the 16-bit torch path and of fp32 on this model was 4.14e-3 in bf16 and 4.61e-4 in fp16 over seeds
0..7 (profiles/moe.txt); MARGIN is 8x that: 3.31e-2 and 3.69e-3. The model's seed (which also draws the tokens) is the first in range(64)
whose fp32 CPU routing has every k-th / (k+1)-th logit gap >= MARGIN. The tokens are drawn from the first four ids of
the 77: with all 77 the 192 decisions of a batch never all clear the bf16 margin (the largest smallest-gap over the 64
seeds is 7.8e-3)."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import transformer_native as TN
from deeplearning4j_amd.ops.gemm import mmul

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
DTS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
G = TN.MOE_ROW_TILE
E, F, X, K = 64, 128, 4, 2


def _err(a, b):
    """The error measure of tests/test_gpu_attention_decode.py."""
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def _bits(t):
    return t.cpu().view(torch.int16) if t.dtype in DTS else t.cpu().view(torch.int32)


def _tol(dt, Kd):
    """tests/test_gpu_gemm.py"""
    return (2e-2 if dt == torch.bfloat16 else 4e-3) * max(1.0, (Kd / 64) ** 0.5)


@functools.lru_cache(maxsize=None)
def _rand(shape, seed, scale=1.0):
    """fp32 on the CPU, never modified."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _planted_logits():
    """N = G + 1 tokens: tokens 0 .. G-1 choose experts (3, 1), the last one (3, 2): cnt = (0, G, 1, G + 1)."""
    l = torch.tensor([0.0, 1.0, -1.0, 2.0]).repeat(G + 1, 1)
    l[G] = torch.tensor([0.0, -1.0, 1.0, 2.0])
    return l


def _planted():
    plan, gate = TN.moe_route(_planted_logits().to(DEV), K)
    return plan, gate


def _plan_lists(plan):
    return {n: getattr(plan, n).cpu().tolist() for n in ("idx", "cnt", "off", "row_of", "src_of", "tile_expert")}


# ------------------------------------------------------------------------------------------------ (a) refusals
def test_the_entry_points_refuse():
    lib = TN._lib()
    p, s = TN._ptr, TN._stream()
    assert lib.dl4j_moe_row_tile() == G
    assert lib.dl4j_moe_rows(G + 1, 2, 4) == TN.moe_rows(G + 1, 2, 4) == 768
    assert lib.dl4j_moe_rows(0, 2, 4) == 0 and lib.dl4j_moe_rows(5, 3, 2) == 0 and lib.dl4j_moe_rows(5, 9, 64) == 0
    assert lib.dl4j_moe_rows(5, 1, 65) == 0 and lib.dl4j_moe_rows(5, 0, 4) == 0
    N, R = 8, TN.moe_rows(8, K, X)
    lg = torch.zeros(N * X + 4, dtype=torch.float32, device=DEV)
    ib = torch.zeros(4096, dtype=torch.int32, device=DEV)
    idx, cnt, off, row_of, src_of, te, ws = ib[:16], ib[16:20], ib[20:25], ib[32:48], ib[64:64 + R], ib[2048:2054], \
        ib[3000:3004]
    gate = torch.zeros(N * K, dtype=torch.float32, device=DEV)
    odd = lambda t: t.data_ptr() + 2  # noqa: E731  not 4-byte aligned
    rt = lib.dl4j_moe_route
    args = lambda **kw: [kw.get(k_, d) for k_, d in (("lg", p(lg)), ("N", N), ("X", X), ("k", K), ("idx", p(idx)),  # noqa: E731
                                                     ("gate", p(gate)), ("cnt", p(cnt)), ("off", p(off)),
                                                     ("row_of", p(row_of)), ("src_of", p(src_of)), ("te", p(te)),
                                                     ("ws", p(ws)))] + [s]
    assert rt(*args()) == 0
    for bad in (dict(N=0), dict(X=0), dict(X=65), dict(k=0), dict(k=5), dict(k=9, X=64), dict(lg=None), dict(idx=None),
                dict(gate=None), dict(cnt=None), dict(off=None), dict(row_of=None), dict(src_of=None), dict(te=None),
                dict(ws=None), dict(lg=odd(lg)), dict(idx=odd(idx)), dict(src_of=odd(src_of))):
        assert rt(*args(**bad)) == -1, bad
    x = torch.zeros(N * E + 16, dtype=torch.bfloat16, device=DEV)
    xp = torch.zeros(R * F + 16, dtype=torch.bfloat16, device=DEV)
    yp = torch.zeros(R * F + 16, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(X * F * F + 16, dtype=torch.bfloat16, device=DEV)
    f32 = torch.zeros(X * F * F + 16, dtype=torch.float32, device=DEV)
    off8 = lambda t: p(t[4:])  # noqa: E731  8 bytes past a 16-byte boundary
    ga = lib.dl4j_moe_gather
    assert ga(1, p(x), p(src_of), p(te), None, p(xp), R, E, K, s) == 0
    assert ga(1, p(x), p(src_of), p(te), p(gate), p(xp), R, E, K, s) == 0
    assert ga(0, p(x), p(src_of), p(te), None, p(xp), R, E, K, s) == -1                   # dtype
    assert ga(1, p(x), p(src_of), p(te), None, p(xp), R, 60, K, s) == -1                  # E % 8
    assert ga(1, p(x), p(src_of), p(te), None, p(xp), R + 8, E, K, s) == -1               # rows % G
    assert ga(1, p(x), p(src_of), p(te), None, p(xp), R, E, 0, s) == -1
    assert ga(1, p(x), p(src_of), p(te), None, p(xp), R, E, 9, s) == -1
    assert ga(1, None, p(src_of), p(te), None, p(xp), R, E, K, s) == -1
    assert ga(1, p(x), None, p(te), None, p(xp), R, E, K, s) == -1
    assert ga(1, p(x), p(src_of), None, None, p(xp), R, E, K, s) == -1
    assert ga(1, p(x), p(src_of), p(te), None, None, R, E, K, s) == -1
    assert ga(1, off8(x), p(src_of), p(te), None, p(xp), R, E, K, s) == -1
    assert ga(1, p(x), p(src_of), p(te), None, off8(xp), R, E, K, s) == -1
    gg = lib.dl4j_gemm_grouped
    ok = lambda **kw: [kw.get(k_, d) for k_, d in (("dt", 1), ("A", p(xp)), ("lda", E), ("B", p(w)), ("ldb", F),  # noqa: E731
                                                   ("bkc", 0), ("sB", E * F), ("C", p(yp)), ("ldc", F),
                                                   ("bias", p(f32)), ("te", p(te)), ("R", R), ("N", F), ("K", E),
                                                   ("X", X))] + [s]
    assert gg(*ok()) == 0 and gg(*ok(bias=None)) == 0 and gg(*ok(bkc=1, ldb=E)) == 0
    for bad in (dict(dt=0), dict(dt=3), dict(A=None), dict(B=None), dict(C=None), dict(te=None), dict(A=off8(xp)),
                dict(B=off8(w)), dict(C=off8(yp)), dict(bias=odd(f32)), dict(R=0), dict(R=R + 8), dict(N=60),
                dict(K=60), dict(lda=E + 4), dict(lda=E - 8), dict(ldb=F + 4), dict(ldb=F - 8), dict(ldc=F - 8),
                dict(sB=E * F + 4), dict(X=0), dict(X=65)):
        assert gg(*ok(**bad)) == -1, bad
    wg = lib.dl4j_gemm_grouped_wgrad
    ok = lambda **kw: [kw.get(k_, d) for k_, d in (("dt", 1), ("A", p(xp)), ("lda", E), ("B", p(yp)), ("ldb", F),  # noqa: E731
                                                   ("dW", p(f32)), ("off", p(off)), ("cnt", p(cnt)), ("R", R),
                                                   ("M", E), ("N", F), ("X", X))] + [s]
    assert wg(*ok()) == 0 and wg(*ok(dW=p(f32[1:]))) == 0                                 # a 4-byte aligned view
    for bad in (dict(dt=0), dict(A=None), dict(B=None), dict(dW=None), dict(off=None), dict(cnt=None),
                dict(A=off8(xp)), dict(B=off8(yp)), dict(dW=odd(f32)), dict(R=R + 8), dict(M=60), dict(N=60),
                dict(lda=E - 8), dict(ldb=F + 4), dict(X=0), dict(X=65)):
        assert wg(*ok(**bad)) == -1, bad
    sc = lib.dl4j_moe_segment_colsum
    assert sc(1, p(yp), p(off), p(cnt), p(f32), X, F, s) == 0
    for a in ((0, p(yp), p(off), p(cnt), p(f32), X, F), (1, None, p(off), p(cnt), p(f32), X, F),
              (1, p(yp), None, p(cnt), p(f32), X, F), (1, p(yp), p(off), None, p(f32), X, F),
              (1, p(yp), p(off), p(cnt), None, X, F), (1, off8(yp), p(off), p(cnt), p(f32), X, F),
              (1, p(yp), p(off), p(cnt), p(f32), X, 60), (1, p(yp), p(off), p(cnt), p(f32), 65, F)):
        assert sc(*a, s) == -1, a
    cb = lib.dl4j_moe_combine
    assert cb(1, p(xp), p(row_of), p(gate), None, p(x), N, E, K, s) == 0
    assert cb(1, p(xp), p(row_of), None, p(x), p(x), N, E, K, s) == 0                     # acc aliases y
    for a in ((0, p(xp), p(row_of), None, None, p(x), N, E, K), (1, None, p(row_of), None, None, p(x), N, E, K),
              (1, p(xp), None, None, None, p(x), N, E, K), (1, p(xp), p(row_of), None, None, None, N, E, K),
              (1, off8(xp), p(row_of), None, None, p(x), N, E, K), (1, p(xp), p(row_of), None, off8(x), p(x), N, E, K),
              (1, p(xp), p(row_of), None, None, off8(x), N, E, K), (1, p(xp), p(row_of), None, None, p(x), 0, E, K),
              (1, p(xp), p(row_of), None, None, p(x), N, 60, K), (1, p(xp), p(row_of), None, None, p(x), N, E, 9)):
        assert cb(*a, s) == -1, a
    bw = lib.dl4j_moe_combine_bwd
    dg = torch.zeros(N * K, dtype=torch.float32, device=DEV)
    assert bw(1, p(x), p(xp), p(row_of), p(dg), N, E, K, s) == 0
    for a in ((0, p(x), p(xp), p(row_of), p(dg), N, E, K), (1, None, p(xp), p(row_of), p(dg), N, E, K),
              (1, p(x), None, p(row_of), p(dg), N, E, K), (1, p(x), p(xp), None, p(dg), N, E, K),
              (1, p(x), p(xp), p(row_of), None, N, E, K), (1, off8(x), p(xp), p(row_of), p(dg), N, E, K),
              (1, p(x), p(xp), p(row_of), p(dg), 0, E, K), (1, p(x), p(xp), p(row_of), p(dg), N, 60, K)):
        assert bw(*a, s) == -1, a
    rb = lib.dl4j_moe_route_bwd
    dl = torch.zeros(N * X, dtype=torch.bfloat16, device=DEV)
    assert rb(1, p(idx), p(gate), p(dg), p(dl), N, X, K, s) == 0
    for a in ((0, p(idx), p(gate), p(dg), p(dl), N, X, K), (1, None, p(gate), p(dg), p(dl), N, X, K),
              (1, p(idx), None, p(dg), p(dl), N, X, K), (1, p(idx), p(gate), None, p(dl), N, X, K),
              (1, p(idx), p(gate), p(dg), None, N, X, K), (1, p(idx), p(gate), p(dg), p(dl), 0, X, K),
              (1, p(idx), p(gate), p(dg), p(dl), N, 65, K), (1, p(idx), p(gate), p(dg), p(dl), N, X, 5)):
        assert rb(*a, s) == -1, a
    torch.cuda.synchronize()
    # the wrappers hand the refusal on as None
    plan, g8 = TN.moe_route(torch.zeros(N, X, device=DEV), K)
    assert TN.moe_route(torch.zeros(N, X, device=DEV, dtype=torch.float64), K) is None
    assert TN.moe_route(torch.zeros(N, X, device=DEV), 5) is None
    assert TN.moe_gather(torch.zeros(N, 60, dtype=torch.bfloat16, device=DEV), plan) is None
    assert TN.moe_gather(torch.zeros(N, E, dtype=torch.float32, device=DEV), plan) is None
    assert TN.gemm_grouped(torch.zeros(plan.rows, 60, dtype=torch.bfloat16, device=DEV),
                           torch.zeros(X, 60, F, dtype=torch.bfloat16, device=DEV), None, plan) is None
    assert TN.moe_combine(torch.zeros(plan.rows, 60, dtype=torch.bfloat16, device=DEV), plan) is None


# ------------------------------------------------------------------------------------------------ (b) route
def _route_case(logits):
    k = _route_case.k
    plan, gate = TN.moe_route(logits.to(DEV), k)
    twin, tgate = TN.moe_route_reference(logits, k)
    got, want = _plan_lists(plan), _plan_lists(twin)
    for name in want:
        assert got[name] == want[name], name
    assert plan.rows == twin.rows == TN.moe_rows(logits.shape[0], k, logits.shape[1])
    l64 = torch.sort(logits.double(), dim=1, descending=True, stable=True).values[:, :k]
    ex = torch.exp(l64 - l64[:, :1])
    g64 = ex / ex.sum(1, keepdim=True)
    rel = ((gate.cpu().double() - g64).abs() / g64).max().item()
    print(f"route N={logits.shape[0]} X={logits.shape[1]} k={k}: gate rel err {rel / 2.0 ** -24:.2f} * 2^-24")
    assert rel <= 4 * 2.0 ** -24
    again, gate2 = TN.moe_route(logits.to(DEV), k)
    assert _plan_lists(again) == got and torch.equal(_bits(gate2), _bits(gate))
    return plan, gate


def test_route_on_the_planted_logits():
    _route_case.k = K
    plan, gate = _route_case(_planted_logits())
    assert plan.cnt.cpu().tolist() == [0, G, 1, G + 1]
    assert plan.off.cpu().tolist() == [0, 0, G, 2 * G, 4 * G]
    assert plan.tile_expert.cpu().tolist() == [1, 2, 3, 3, -1, -1]
    assert plan.idx[0].cpu().tolist() == [3, 1] and plan.idx[G].cpu().tolist() == [3, 2]


@pytest.mark.parametrize("x,k,n", [(8, 2, 200), (64, 8, 70), (4, 1, 3), (8, 2, 1), (4, 2, 700)])
@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
def test_route_equals_the_torch_twin(x, k, n, ties):
    logits = _rand((n, x), 7 * n + x).clone()
    if ties:
        logits[::3] = torch.round(logits[::3])
        logits[1::5, : max(2, x // 2)] = 2.0
    _route_case.k = k
    _route_case(logits)


# ------------------------------------------------------------------------------------------------ (c) grouped GEMM
def _live_reference(xp, w64, bias, plan):
    """fp64 [rows, N] of every live row with its own expert's matrix (dead / pad rows: NaN) and the live mask."""
    L = _plan_lists(plan)
    out = torch.full((plan.rows, w64.shape[2]), float("nan"), dtype=torch.float64)
    x64 = xp.cpu().double()
    for r, src in enumerate(L["src_of"]):
        if src >= 0:
            e = L["tile_expert"][r // G]
            out[r] = x64[r] @ w64[e] + (bias[e].double() if bias is not None else 0)
    return out, torch.tensor([s >= 0 for s in L["src_of"]])


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kd,nd", [(64, 128), (200, 128), (64, 200), (200, 72)])
@pytest.mark.parametrize("bkc", [False, True], ids=["Ncontig", "Kcontig"])
def test_grouped_gemm_against_fp64(dt, kd, nd, bkc):
    plan, _ = _planted()
    n = G + 1
    x = _rand((n, kd), 1).to(dt).to(DEV)
    xp = TN.moe_gather(x, plan)
    w = _rand((X, kd, nd), 2, kd ** -0.5).to(dt)
    bias = _rand((X, nd), 3).to(DEV)
    wd = w.transpose(1, 2).contiguous().to(DEV).transpose(1, 2) if bkc else w.to(DEV)
    c = torch.full((plan.rows, nd), 7.0, dtype=dt, device=DEV)
    assert TN.gemm_grouped(xp, wd, bias, plan, out=c) is c
    ref, live = _live_reference(xp, w.double(), bias.cpu(), plan)
    scale = ref[live].abs().max().item()
    err = (c.cpu().double()[live] - ref[live]).abs().max().item()
    print(f"grouped gemm {dt} K={kd} N={nd} bkc={bkc}: err {err:.3e} scale {scale:.3f} bound {_tol(dt, kd) * scale:.3e}")
    assert err <= _tol(dt, kd) * scale
    dead = torch.tensor(_plan_lists(plan)["tile_expert"]).repeat_interleave(G) < 0
    assert dead.sum() == 2 * G and bool((c.cpu()[dead] == 7.0).all())
    # a subset of the tokens: the same bits per token
    keep = list(range(0, 40)) + [G]
    sub, _ = TN.moe_route(_planted_logits()[keep].to(DEV), K)
    c2 = TN.gemm_grouped(TN.moe_gather(x[keep].contiguous(), sub), wd, bias, sub)
    a = c[plan.row_of.long()[keep].reshape(-1)]
    b = c2[sub.row_of.long().reshape(-1)]
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ (d) pad rows
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_nan_in_pad_rows_and_dead_tiles_changes_no_bit(dt):
    plan, gate = _planted()
    n = G + 1
    x = _rand((n, E), 4).to(dt).to(DEV)
    w1 = _rand((X, E, F), 5, E ** -0.5).to(dt).to(DEV)
    w2 = _rand((X, F, E), 6, F ** -0.5).to(dt).to(DEV)
    b2 = _rand((X, E), 8).to(DEV)
    pad = (plan.src_of < 0).unsqueeze(1)

    def run(fill):
        poison = lambda t: torch.where(pad, torch.full_like(t, fill), t)  # noqa: E731
        xp = poison(TN.moe_gather(x, plan))
        fp = poison(TN.gemm_grouped(xp, w1, None, plan))
        yp = TN.gemm_grouped(fp, w2, b2, plan)
        y = TN.moe_combine(yp, plan, gate)
        dz = poison(TN.gemm_grouped(xp, w1, None, plan))
        dw = torch.empty(X * E, F, dtype=torch.float32, device=DEV)
        TN.gemm_grouped_wgrad(xp, dz, plan, dw)
        db = torch.empty(X, F, dtype=torch.float32, device=DEV)
        TN.moe_segment_colsum(dz, plan, db)
        return y, dw, db
    zero, nan = run(0.0), run(float("nan"))
    for a, b in zip(zero, nan):
        assert bool(torch.isfinite(b).all()) and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ (e) wgrad, sums
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_grouped_wgrad_and_segment_sums_against_fp64(dt):
    plan, _ = _planted()
    L = _plan_lists(plan)
    n = G + 1
    ap = TN.moe_gather(_rand((n, E), 9).to(dt).to(DEV), plan)
    bp = TN.moe_gather(_rand((n, F), 10).to(dt).to(DEV), plan)
    dw = torch.full((X * E, F), 5.0, dtype=torch.float32, device=DEV)
    db = torch.full((X, F), 5.0, dtype=torch.float32, device=DEV)
    assert TN.gemm_grouped_wgrad(ap, bp, plan, dw) is dw and TN.moe_segment_colsum(bp, plan, db) is db
    a64, b64 = ap.cpu().double(), bp.cpu().double()
    for e in range(X):
        seg = slice(L["off"][e], L["off"][e] + L["cnt"][e])
        want, got = a64[seg].t() @ b64[seg], dw[e * E:(e + 1) * E].cpu().double()
        sums = b64[seg].sum(0)
        if L["cnt"][e] == 0:
            assert bool((got == 0).all()) and bool((db[e] == 0).all())
            continue
        scale, s2 = want.abs().max().item(), sums.abs().max().item()
        err, e2 = (got - want).abs().max().item(), (db[e].cpu().double() - sums).abs().max().item()
        print(f"wgrad {dt} expert {e} cnt {L['cnt'][e]}: err {err:.3e} of {scale:.3f}, colsum err {e2:.3e} of {s2:.3f}")
        assert err <= _tol(dt, L["cnt"][e]) * scale and e2 <= _tol(dt, L["cnt"][e]) * s2
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    TN.gemm_grouped_wgrad(ap, bp, plan, dw2)
    TN.moe_segment_colsum(bp, plan, db2)
    assert torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2))


# ------------------------------------------------------------------------------------------------ (f) combine
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_combine_its_backward_and_the_route_backward(dt):
    n, x, k = 200, 8, 2
    plan, gate = TN.moe_route(_rand((n, x), 11).to(DEV), k)
    yp = _rand((plan.rows, E), 12).to(dt).to(DEV)
    acc = _rand((n, E), 13).to(dt).to(DEV)
    rows = plan.row_of.long().cpu()
    y64 = yp.cpu().double()[rows.reshape(-1)].reshape(n, k, E)
    g64 = gate.cpu().double()
    terms = g64.unsqueeze(2) * y64
    for a in (None, acc):
        y = TN.moe_combine(yp, plan, gate, a)
        want = terms.sum(1) + (0 if a is None else a.cpu().double())
        bound = 1.01 * U[dt] * (terms.abs().sum(1) + (0 if a is None else a.cpu().double().abs()))
        assert bool(((y.cpu().double() - want).abs() <= bound).all())
    alias = acc.clone()
    assert TN.moe_combine(yp, plan, gate, alias, out=alias) is alias
    assert torch.equal(_bits(alias), _bits(TN.moe_combine(yp, plan, gate, acc)))
    ones = TN.moe_combine(yp, plan, None, None)
    assert bool(((ones.cpu().double() - y64.sum(1)).abs() <= 1.01 * U[dt] * y64.abs().sum(1)).all())
    dy = _rand((n, E), 14).to(dt).to(DEV)
    dgate = TN.moe_combine_bwd(dy, yp, plan)
    prod = dy.cpu().double().unsqueeze(1) * y64
    assert bool(((dgate.cpu().double() - prod.sum(2)).abs() <= E * 2.0 ** -24 * prod.abs().sum(2)).all())
    assert torch.equal(_bits(dgate), _bits(TN.moe_combine_bwd(dy, yp, plan)))
    dl = TN.moe_route_bwd(plan, gate, dgate, dt)
    d64 = dgate.cpu().double()
    want = torch.zeros(n, x, dtype=torch.float64)
    want.scatter_(1, plan.idx.long().cpu(), g64 * (d64 - (g64 * d64).sum(1, keepdim=True)))
    # one rounding to the 16-bit type (U relative) on top of the fp32 evaluation of g * (d - s), which can cancel: with
    # D = max_j |d_j| of the token, s = g_0 d_0 + g_1 d_1 carries 3 roundings of values <= D, d - s one of a value
    # <= 2D, the product and the fp32 gate one each of values <= 2D: at most 9 * 2^-24 * D before the 16-bit rounding
    dmax = d64.abs().max(1, keepdim=True).values
    assert bool(((dl.cpu().double() - want).abs() <= 1.01 * U[dt] * want.abs() + 9 * 2.0 ** -24 * dmax).all())
    assert bool((dl.cpu()[want == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ (g) model
V = 77
MARGIN = {DataType.BFLOAT16: 8 * 4.14e-3, DataType.HALF: 8 * 4.61e-4}
NET_DTS = [DataType.BFLOAT16, DataType.HALF]
BLOCKS = ("decoder_0", "decoder_1")


def _lm(dt, device, seed, **kw):
    return TextGenerationTransformer(numLabels=V, hidden=128, layers=2, heads=2, nKVHeads=1, ffn=128, inputShape=[32],
                                     maxPositions=96, seed=seed, dataType=dt, positionEncoding="rotary",
                                     normalization="rms", normPlacement="pre", ffnActivation="swiglu", nExperts=4,
                                     nExpertsPerToken=2, **kw).init(device=device)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (3, 32), generator=g)
    y = torch.zeros(3, V, 32)
    y.scatter_(1, torch.randint(0, V, (3, 1, 32), generator=g), 1.0)
    return x, y


def _spy(net):
    """Record (router logits fp32, idx) of every sparse block's feed-forward calls -> the list, and an undo."""
    rec = []
    for name in BLOCKS:
        layer = net.layers_by_name[name]

        def fwd(n, acc=None, layer=layer, orig=layer._moe_fwd):
            sixteen = n.dtype in DTS
            logits = mmul(n, layer.W("Wr"), out_dtype=torch.float32 if sixteen else None)
            out = orig(n, acc)
            rec.append((logits.float().cpu(), out[1][0].idx.cpu()))
            return out
        layer._moe_fwd = fwd

    def undo():
        for name in BLOCKS:
            del net.layers_by_name[name]._moe_fwd
    return rec, undo


def _gap(logits, k=2):
    s = torch.sort(logits, dim=1, descending=True).values
    return float((s[:, k - 1] - s[:, k]).min())


@functools.lru_cache(maxsize=None)
def _reference(dt):
    """(seed, the fp32 CPU net, its routing [(logits, idx)] on the seed's batch): the first seed whose every routing
    decision clears MARGIN."""
    for seed in range(64):
        cpu = _lm(DataType.FLOAT, CPU, seed)
        rec, undo = _spy(cpu)
        cpu.output(_batch(seed)[0])
        undo()
        if min(_gap(l) for l, _ in rec) >= MARGIN[dt]:
            return seed, cpu, rec
    pytest.fail(f"no seed in range(64) whose routing clears the margin {MARGIN[dt]}")


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.to(dst.flattenedParams.device))
    dst._params_changed()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


@pytest.mark.parametrize("dt", NET_DTS, ids=IDS)
def test_routing_and_training_step_match_fp32_cpu(dt):
    """The measure and bound of tests/test_gpu_llama_block.py: gradient rel L2 < 3e-2, score within 3e-2."""
    seed, cpu, want = _reference(dt)
    gpu = _lm(dt, DEV, seed)
    _copy_params(gpu, cpu)
    x, y = _batch(seed)
    rec, undo = _spy(gpu)
    fallback.reset()
    gpu.computeGradientAndScore([x.to(DEV)], [y.to(DEV)])
    torch.cuda.synchronize()
    undo()
    assert gpu.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    assert len(rec) == len(want) == 2
    for (lg, ig), (lc, ic) in zip(rec, want):
        print(f"moe model {dt} seed {seed}: router logits max diff {float((lg - lc).abs().max()):.3e}, "
              f"smallest gap {_gap(lc):.3e}")
        assert torch.equal(ig, ic)
    cpu.computeGradientAndScore([x], [y])
    ga, gb = gpu.flattenedGradients.float().cpu(), cpu.flattenedGradients.float()
    rel = float((ga - gb).norm() / gb.norm())
    print(f"moe training step {dt}: gradient rel {rel:.3e}, scores {gpu.score():.5f} {cpu.score():.5f}")
    assert rel < 3e-2, rel
    assert abs(gpu.score() - cpu.score()) < 3e-2 * abs(cpu.score())


@pytest.mark.parametrize("dt", NET_DTS, ids=IDS)
def test_generation_end_to_end(dt):
    N = 12
    seed, cpu, _ = _reference(dt)
    gpu = _lm(dt, DEV, seed)
    _copy_params(gpu, cpu)
    prompt = _batch(seed)[0][:, :5].contiguous()
    fallback.reset()
    r = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    toks = r.tokens.cpu()
    # the fp32 CPU loop fed the same tokens: every step's distribution (rel L2 < 3e-2, as the llama test)
    gpu.rnnClearPreviousState()
    cpu.rnnClearPreviousState()
    og, oc = gpu.rnnTimeStep(prompt.to(DEV))[0], cpu.rnnTimeStep(prompt)[0]
    for i in range(N):
        assert _rel(og[:, :, -1], oc[:, :, -1]) < 3e-2, i
        assert torch.equal(og[:, :, -1].argmax(1).cpu(), toks[:, i])
        og, oc = gpu.rnnTimeStep(toks[:, i:i + 1].to(DEV))[0], cpu.rnnTimeStep(toks[:, i:i + 1])[0]
    pinned = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0, pinPositions=True)
    assert torch.equal(pinned.tokens, r.tokens)
    graph = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0, useGraph=True)
    stats = gpu.lastGenerationStats
    assert torch.equal(graph.tokens, pinned.tokens) and torch.equal(_bits(graph.scores), _bits(pinned.scores))
    assert stats["captures"] == 1 and stats["graphReplays"] > 0
    assert fallback.count() == 0 and gpu.helperCountFail() == 0, fallback.summary()
    # the fp8 cache and ragged prompts run on the kernels too
    lens = [5, 3, 4]
    ragged = gpu.generate(prompt.to(DEV), promptLengths=lens, maxNewTokens=N)
    for b, n in enumerate(lens):
        alone = gpu.generate(prompt[b:b + 1, :n].contiguous().to(DEV), maxNewTokens=N)
        assert torch.equal(ragged.tokens[b:b + 1], alone.tokens), f"row {b} ({n} tokens)"
    gpu.rnnClearPreviousState()
    gpu.rnnSetCacheDataType("fp8")
    r8 = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert r8.tokens.shape == r.tokens.shape and fallback.count() == 0, fallback.summary()


# the profiler method and the rule of tests/test_gpu_llama_block.py
def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


def _profiled(step, warm=2):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_a_training_step_launches_no_torch_compute_kernels():
    net = _lm(DataType.BFLOAT16, DEV, 0)
    x, y = _batch(0)
    x, y = x.to(DEV), y.to(DEV)
    fallback.reset()
    names = _profiled(lambda: net.fit([x], [y]))
    assert sum("moe_topk_kernel" in n for n in names) == 2 and sum("moe_route_bwd_kernel" in n for n in names) == 2
    torch_ks = sorted({n for n in names if _is_torch_kernel(n)})
    assert not torch_ks, f"torch compute kernels in the training step: {torch_ks[:6]}"
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()


_ALLOWED = ("bfloat16tofloat32_copy_kernel",)


def test_a_decode_step_launches_no_torch_compute_kernels():
    """The decode step of this model (batch 4) was 38 launches when the test was written; a block's sparse
    feed-forward is 9 of them: the router GEMM, the three routing kernels, the gather, two grouped GEMMs with the
    swiglu between them, and the combine that also adds the residual."""
    net = _lm(DataType.BFLOAT16, DEV, 0)
    x = torch.randint(0, V, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    it = iter(steps)
    names = _profiled(lambda: net.rnnTimeStep(next(it)))
    print(f"moe decode step: {len(names)} launches")
    assert sum("moe_topk_kernel" in n for n in names) == 2 and sum("moe_combine_kernel" in n for n in names) == 2
    assert sum("moe_gather_kernel" in n for n in names) == 2
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
