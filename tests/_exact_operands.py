"""Operands on which a GEMM has no rounding to hide behind, shared by tests/test_exact_operands.py (CPU) and
tests/test_gpu_gemm_exact.py (GPU) so that the two cannot drift apart.

With small integers, or values of an MX grid times powers of two, every product x * w is exact and every partial sum,
in any order, is a multiple of one power of two q below 2^24 q: an fp32 value. A kernel's fp32 accumulator then holds
the mathematically exact sum whatever its wave, chunk and split order, and its output must be the fp64 product rounded
ONCE to the output type, bit for bit. ``assert_exact`` checks that premise for a given product, ``expected`` does the
one rounding.

Everything here is made on the CPU from generators seeded by the case's own key, cached, and never modified."""
import functools
import zlib

import numpy as np
import torch

E2M1 = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)          # the nonzero e2m1 magnitudes
DTS = (torch.bfloat16, torch.float16)
X, TOPK = 4, 2                                      # experts and choices per token of the grouped products

# ---- the shapes of tests/test_gpu_gemm_exact.py
SKINNY_M = (1, 16, 17, 33, 64)
SKINNY_K = (8, 40, 127, 128, 129, 264, 520)         # vector, 32-deep step, the 128 / 256 chunk edges, ragged tails
SKINNY_N = (8, 24, 77, 136, 200)
SKINNY_SPLIT_K = 520                                # must run split on every layout (asserted through the workspace)
SKINNY_LONG = ((3, 3072, 80), (3, 768, 2304))       # (M, K, N): where the tolerance tests are blind
GROUPED_KN = ((40, 24), (129, 77), (520, 136))
GROUPED_SPLIT_KN = (520, 136)
GROUPED_NTOK = (1, 5, 17, 64)
PLANS = ("last_idle", "first_and_middle_idle")
# the quantised formats take K % 32 == 0 only (groups of 32 along K): 264 and 520 are refused by the format itself, so
# the products run at the next multiples of 32; the refusal of the two is asserted
WQ_KN = ((32, 16), (96, 77), (288, 40), (544, 33))
WQ_REFUSED_KN = ((264, 40), (520, 33))
WQ_SPLIT_K = 288                                    # the smallest K that wq_split of csrc/gemm_wq.hip can split
FMTS = ("fp8", "fp4")
MMUL_SHAPES = ((552, 328, 384), (136, 72, 200))     # (M, N, K); the second has a K tail
MMUL_CFGS = ((0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (4, 3), (2, 2), (5, 1), (8, 1), (9, 1), (3, 3), (7, 2))
MMUL_ODD = ((3, 5, 7), (33, 17, 9), (130, 1, 70))
STREAM_M = 128 * 40
STREAM_NK = ((256, 64), (512, 64), (128, 64), (256, 128), (512, 256), (64, 64), (64, 128), (64, 256), (128, 512),
             (192, 64))
MOE_G = 128                                         # the row tile of the grouped MFMA GEMM
MOE_KN = ((64, 128), (200, 128), (64, 200), (200, 72))
GELU_MAX = 8.0                                      # |pre-activation| of the GELU cases


def gen(*key):
    """A generator seeded by the case's key alone."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(shape, lo, hi, g):
    """fp64 nonzero integers with magnitude in [lo, hi] and random sign: a dropped term always moves the sum."""
    n = hi - lo + 1
    r = torch.randint(0, 2 * n, shape, generator=g, dtype=torch.int32)           # one draw: magnitude and sign
    return torch.where(r < n, r + lo, n - r - lo).double()


def mx_grid_weights(fmt, K, N, g, exps=(-3, 3)):
    """fp64 [K, N] on ``fmt``'s grid: e2m1 magnitudes, or integers up to 16 for e4m3, with random sign, times 2^e with
    an independent e in ``exps`` per 32-deep k group and column, so neighbouring groups and neighbouring columns carry
    different scale bytes and quantisation loses nothing."""
    if fmt == "fp4":
        mag = torch.tensor(E2M1, dtype=torch.float64)[torch.randint(0, len(E2M1), (K, N), generator=g)]
    else:
        mag = torch.randint(1, 17, (K, N), generator=g).double()
    sign = (torch.randint(0, 2, (K, N), generator=g) * 2 - 1).double()
    e = torch.randint(exps[0], exps[1] + 1, (K // 32, N), generator=g).double()
    return mag * sign * torch.exp2(e).repeat_interleave(32, dim=0)


def quantum(*tensors):
    """The largest power of two that divides every value of the tensors (multiples of 2^-40 below 2^22): the lowest
    bit set in any of them."""
    every = 0
    for t in tensors:
        fixed = t.double().abs() * 2.0 ** 40
        assert torch.equal(fixed, fixed.round()) and fixed.max().item() < 2.0 ** 62
        every |= int(np.bitwise_or.reduce(fixed.to(torch.int64).numpy().reshape(-1)))
    assert every, "all zeros"
    return (every & -every) * 2.0 ** -40


def assert_exact(x, w, extra, dt):
    """What makes "bit-equal" legitimate for out = x [M, K] @ w [K, N] + extra (the sum of the epilogue's terms, or
    None) in output type ``dt``. Every product is a multiple of quantum(x) * quantum(w), so with q the smaller of that
    and quantum(extra): (|x| @ |w| + |extra|).max() / q < 2^24, every partial sum in any order is an fp32 value; and
    max|out| < 65504 for fp16, no output overflows. The operands themselves must be values of the 16-bit type."""
    x, w = x.double(), w.double()
    q = quantum(x) * quantum(w)
    top = x.abs() @ w.abs()
    ref = x @ w
    if extra is not None:
        extra = extra.double()
        q = min(q, quantum(extra))
        top, ref = top + extra.abs(), ref + extra
    assert top.max().item() / q < 2 ** 24, f"partial sums reach {top.max().item() / q:.0f} quanta of {q}"
    for d in (dt if isinstance(dt, (tuple, list)) else (dt,)):                  # one output type or several
        if d == torch.float16:
            assert ref.abs().max().item() < 65504
        if d != torch.float32:
            for t in (x, w):
                assert torch.equal(t.to(d).double(), t), f"an operand is no {d} value"


def expected(ref64, dt):
    """The fp64 result rounded once to the output type."""
    return ref64.float() if dt == torch.float32 else ref64.to(dt)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def dense(M, K, N, xhi=4, whi=8):
    """(x [M, K], w [K, N], bias [N], c0 [M, N]): integers. The long-K shapes narrow the ranges."""
    g = gen("dense", M, K, N)
    if K >= 768:
        xhi, whi = 2, 4
    return ints((M, K), 1, xhi, g), ints((K, N), 1, whi, g), ints((N,), 1, 8, g), ints((M, N), 1, 8, g)


@functools.lru_cache(maxsize=None)
def mx(fmt, M, K, N):
    """(x, w on the MX grid, bias, c0)."""
    g = gen("mx", fmt, M, K, N)
    return ints((M, K), 1, 4, g), mx_grid_weights(fmt, K, N, g), ints((N,), 1, 8, g), ints((M, N), 1, 8, g)


@functools.lru_cache(maxsize=None)
def grouped(fmt, K, N, Ntok):
    """(x [Ntok, K], w [X, K, N] with every expert drawn on its own, bias [X, N]); fmt None: integers."""
    g = gen("grouped", fmt, K, N, Ntok)
    x = ints((Ntok, K), 1, 4, g)
    w = torch.stack([ints((K, N), 1, 8, g) if fmt is None else mx_grid_weights(fmt, K, N, g) for _ in range(X)])
    return x, w, ints((X, N), 1, 8, g)


@functools.lru_cache(maxsize=None)
def plan(kind, Ntok):
    """The routing plan (the reference router's, on the CPU) of planted logits. "last_idle": expert 0 owns every
    token, experts 1 / 2 the even / odd ones, expert 3 none (2 none either at one token).
    "first_and_middle_idle": cnt = (0, Ntok, 0, Ntok)."""
    from deeplearning4j_amd.ops import transformer_native as TN
    logits = torch.zeros(Ntok, X)
    if kind == "last_idle":
        logits[:, 0], logits[:, 3] = 4.0, -4.0
        even = torch.arange(Ntok) % 2 == 0
        logits[:, 1], logits[:, 2] = torch.where(even, 2.0, 1.0), torch.where(even, 1.0, 2.0)
        want = [Ntok, (Ntok + 1) // 2, Ntok // 2, 0]
    else:
        logits[:, 0], logits[:, 1], logits[:, 2], logits[:, 3] = -4.0, 2.0, -3.0, 1.0
        want = [0, Ntok, 0, Ntok]
    p = TN.moe_route_reference(logits, TOPK)[0]
    assert p.cnt.tolist() == want
    return p


def grouped_rows(p, x):
    """(a [rows, K]: the x row every sorted row multiplies, live [rows])."""
    src = p.src_of.long()
    return x[src.clamp_min(0) // p.k], src >= 0


def grouped_reference(p, a, w, bias):
    """fp64 [rows, N]: every expert's segment times its own matrix, plus its bias; zeros elsewhere."""
    ref = torch.zeros(p.rows, w.shape[2], dtype=torch.float64)
    for e in range(p.X):
        seg = slice(int(p.off[e]), int(p.off[e]) + int(p.cnt[e]))
        ref[seg] = a[seg] @ w[e] + bias[e]
    return ref


@functools.lru_cache(maxsize=None)
def moe_planted_logits():
    """tests/test_gpu_moe.py's planted routing: cnt = (0, G, 1, G + 1)."""
    l = torch.tensor([0.0, 1.0, -1.0, 2.0]).repeat(MOE_G + 1, 1)
    l[MOE_G] = torch.tensor([0.0, -1.0, 1.0, 2.0])
    return l


@functools.lru_cache(maxsize=None)
def moe(K, N):
    """(x [G + 1, K], w [X, K, N], bias [X, N]) of the grouped MFMA GEMM."""
    g = gen("moe", K, N)
    return ints((MOE_G + 1, K), 1, 4, g), torch.stack([ints((K, N), 1, 8, g) for _ in range(X)]), ints((X, N), 1, 8, g)


def gelu_scaled(x, w, extra=None):
    """w and extra times the power of two that brings every pre-activation x @ w + extra into [-GELU_MAX, GELU_MAX]:
    still exact, and inside the range where the device GELU's error was measured."""
    z = x @ w + (0 if extra is None else extra)
    s = 1.0
    while z.abs().max().item() * s > GELU_MAX:
        s /= 2
    return w * s, (None if extra is None else extra * s)


# ------------------------------------------------------------------------------------- every product the GPU file runs
def products():
    """(label, x, w, extra, output types, format or None) of every product tests/test_gpu_gemm_exact.py launches; the
    epilogue terms enter ``extra`` at their largest (bias and beta = 1)."""
    for M in SKINNY_M:
        for K in SKINNY_K:
            for N in SKINNY_N:
                x, w, b, c0 = dense(M, K, N)
                yield f"skinny {M}x{K}x{N}", x, w, b.abs() + c0.abs(), DTS, None
    for M, K, N in SKINNY_LONG:
        x, w, b, c0 = dense(M, K, N)
        yield f"skinny {M}x{K}x{N}", x, w, b.abs() + c0.abs(), (torch.bfloat16,), None
    for fmt in (None,) + FMTS:
        for K, N in (GROUPED_KN if fmt is None else WQ_KN):
            for Ntok in GROUPED_NTOK:
                x, w, b = grouped(fmt, K, N, Ntok)
                for e in range(X):
                    yield f"grouped {fmt} {Ntok}x{K}x{N} expert {e}", x, w[e], b[e].abs().expand(Ntok, N), DTS, fmt
    for fmt in FMTS:
        for K, N in WQ_KN:
            for M in SKINNY_M:
                x, w, b, c0 = mx(fmt, M, K, N)
                yield f"wq {fmt} {M}x{K}x{N}", x, w, b.abs() + c0.abs(), DTS, fmt
    for M, N, K in MMUL_SHAPES + MMUL_ODD:
        x, w, b, c0 = dense(M, K, N)
        yield f"mmul {M}x{N}x{K}", x, w, b.abs() + c0.abs(), DTS + (torch.float32,), None
    for M, N, K in MMUL_SHAPES:
        x, w, _, _ = dense(M, K, N, 64, 64)
        yield f"mmul fp32 {M}x{N}x{K}", x, w, None, (torch.float32,), None
    for N, K in STREAM_NK:
        x, w, b, _ = dense(STREAM_M, K, N)
        yield f"stream {N}x{K}", x, w, b.abs(), DTS, None
    for K, N in MOE_KN:
        x, w, b = moe(K, N)
        for e in range(X):
            yield f"moe {K}x{N} expert {e}", x, w[e], b[e].abs().expand(x.shape[0], N), DTS, None
