"""Skinny 16-bit decoding products on the GPU (csrc/gemm_skinny.hip): the dense product on both weight layouts and the
grouped product per expert against fp64 with the error measure and bound of tests/test_gpu_gemm.py, and language
models decoding under rnnSetWeightDataType("native") against the same parameters on the default path."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTS = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
X, TOPK = 4, 2
NAN = float("nan")


def _tol(dt, K):
    """tests/test_gpu_gemm.py's bound for 16-bit operands."""
    return (2e-2 if dt == torch.bfloat16 else 4e-3) * max(1.0, (K / 64) ** 0.5)


@functools.lru_cache(maxsize=None)
def _weights(dt, K, N):
    """W [K, N] on the CPU, never modified."""
    return (torch.randn(K, N, generator=torch.Generator().manual_seed(K + N)) * 0.05).to(dt)


def _on_gpu(w, layout):
    """The same values as an N-contiguous or a K-contiguous view."""
    return w.to(DEV) if layout == "n" else w.t().contiguous().to(DEV).t()


@pytest.mark.parametrize("M,beta,act", [(1, 0.0, None), (3, 1.0, None), (16, 0.0, "gelu"), (17, 1.0, "gelu"),
                                        (64, 0.0, None), (65, 1.0, "gelu")])
@pytest.mark.parametrize("K,N,layout", [(8, 8, "n"), (8, 8, "k"), (40, 24, "n"), (40, 24, "k"), (96, 77, "k"),
                                        (768, 2304, "n"), (768, 2304, "k"), (3072, 80, "n"), (3072, 80, "k")])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_skinny_gemm_against_fp64(dt, K, N, layout, M, beta, act):
    """One partial k step, a K tail that is no multiple of 32, masked tail columns, a split-K shape, a single ragged
    column block. Up to 64 rows the kernel itself (skinny_linear hands only the row counts at which it pays to it);
    M = 65 takes mmul through skinny_linear."""
    w = _weights(dt, K, N)
    if K == 768 and M <= 64:
        assert TN._lib().dl4j_skinny_gemm_workspace(0, M, N, K, *((N, 1) if layout == "n" else (1, K))) > 0
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(dt)
    bias = torch.randn(N, generator=g) if M != 16 else torch.randn(N, generator=g).to(dt)    # fp32 master or 16-bit
    c0 = torch.randn(M, N, generator=g).to(dt)
    ref = x.double() @ w.double() + bias.double() + beta * c0.double()
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    wg = _on_gpu(w, layout)
    runs = []
    for _ in range(2):
        buf = torch.full((M + 2, N + 5), NAN, dtype=dt, device=DEV)                # rows after M, columns after N
        out = buf[:M, :N]
        if beta:
            out.copy_(c0)
        fallback.reset()
        r = (TN.skinny_gemm if M <= 64 else TN.skinny_linear)(x.to(DEV), wg, bias.to(DEV), act, out, beta)
        assert r is out and fallback.count() == 0, fallback.summary()
        host = buf.cpu()
        assert host[M:].isnan().all() and host[:, N:].isnan().all(), "nothing outside [M, N] changes"
        runs.append(host[:M, :N])
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), "two runs give the same bits"
    err = (runs[0].double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{dt} {layout} M={M} K={K} N={N}: max err {err:.3e}, bound {_tol(dt, K) * scale:.3e}")
    assert err <= _tol(dt, K) * scale


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_both_load_widths_of_the_n_contiguous_layout(dt, width):
    """The rule picks one width per shape; the other stays reachable and right: K and N tails, 33 rows."""
    K, N, M = 424, 200, 33
    w = _weights(dt, K, N)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).to(dt)
    ref = x.double() @ w.double()
    buf = torch.full((M + 2, N + 8), NAN, dtype=dt, device=DEV)       # aligned rows: the vector stores
    got = TN.skinny_gemm(x.to(DEV), w.to(DEV), out=buf[:M, :N], width=width)
    assert got is not None
    host = buf.cpu()
    assert host[M:].isnan().all() and host[:, N:].isnan().all()
    assert (host[:M, :N].double() - ref).abs().max() <= _tol(dt, K) * ref.abs().max()


@functools.lru_cache(maxsize=None)
def _plan(Ntok):
    """Expert 0 owns every token, expert 3 none; experts 1 / 2 take the even / odd tokens (2 none at Ntok = 1)."""
    logits = torch.zeros(Ntok, X)
    logits[:, 0], logits[:, 3] = 4.0, -4.0
    even = torch.arange(Ntok) % 2 == 0
    logits[:, 1], logits[:, 2] = torch.where(even, 2.0, 1.0), torch.where(even, 1.0, 2.0)
    plan = TN.moe_route_reference(logits, TOPK)[0]
    assert plan.cnt.tolist() == [Ntok, (Ntok + 1) // 2, Ntok // 2, 0]
    return plan


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "sorted"])
@pytest.mark.parametrize("Ntok", [1, 5, 64])
@pytest.mark.parametrize("K,N", [(64, 48), (768, 256)])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_grouped_skinny_gemm_against_fp64(dt, K, N, Ntok, gather):
    """The gathered product carries the GELU epilogue (W1), the sorted one none (W2); the sorted input holds NaN in
    every row that no assignment owns: pad rows enter as zeros."""
    w = _weights(dt, X * K, N)                                       # the stacked parameter
    plan = _plan(Ntok)
    if K == 768:
        assert TN._lib().dl4j_skinny_gemm_grouped_workspace(0, Ntok, TOPK, X, N, K) > 0
    g = torch.Generator().manual_seed(Ntok + K)
    bias = torch.randn(X, N, generator=g)
    src = plan.src_of.long()
    live = src >= 0
    rows_x = torch.randn(Ntok, K, generator=g).to(dt)
    a = rows_x[src.clamp_min(0) // TOPK]                                     # the row every sorted row multiplies
    x = rows_x if gather else torch.where(live.unsqueeze(1), a, torch.full_like(a, NAN))
    ref = torch.zeros(plan.rows, N, dtype=torch.float64)
    for e in range(X):
        seg = slice(int(plan.off[e]), int(plan.off[e]) + int(plan.cnt[e]))
        ref[seg] = a[seg].double() @ w[e * K:(e + 1) * K].double() + bias[e].double()
    if gather:
        ref = torch.nn.functional.gelu(ref)
    gpu_plan = plan._replace(**{f: getattr(plan, f).to(DEV) for f in ("cnt", "off", "src_of")})
    wg = w.to(DEV).view(X, K, N)
    runs = []
    for _ in range(2):
        buf = torch.full((plan.rows + 2, N + 5), NAN, dtype=dt, device=DEV)
        out = buf[:plan.rows, :N]
        fallback.reset()
        r = TN.skinny_gemm_grouped(x.to(DEV), wg, bias.to(DEV), gpu_plan, gather, "gelu" if gather else None, out)
        assert r is out and fallback.count() == 0, fallback.summary()
        host = buf.cpu()
        assert host[plan.rows:].isnan().all() and host[:, N:].isnan().all(), "nothing outside [Rcap, N] changes"
        assert host[:plan.rows][~live].isnan().all(), "pad rows and idle experts' segments are never written"
        runs.append(host[:plan.rows, :N][live])
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), "two runs give the same bits"
    err = (runs[0].double() - ref[live]).abs().max().item()
    scale = ref[live].abs().max().item()
    print(f"{dt} Ntok={Ntok} K={K} N={N} gather={gather}: max err {err:.3e}, bound {_tol(dt, K) * scale:.3e}")
    assert err <= _tol(dt, K) * scale


V = 77
LLAMA = dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu", positionEncoding="rotary")
STYLES = {"bert": {}, "llama": LLAMA, "moe": dict(nExperts=X, nExpertsPerToken=TOPK, **LLAMA)}


def _lm(style, fmt=None, seed=5):
    return TextGenerationTransformer(numLabels=V, hidden=128, layers=2, heads=2, inputShape=[16], maxPositions=96,
                                     seed=seed, dataType=DataType.BFLOAT16, weightDataType=fmt,
                                     expertWeightDataType=fmt if style == "moe" else None,
                                     **STYLES[style]).init(device=DEV)


def _is_torch_kernel(name):                     # the rule of tests/test_gpu_step_kernels.py
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


def _step_kernels(net, x):
    """Kernel names of the third decode step (the profiler method of tests/test_gpu_llama_block.py)."""
    from torch.profiler import ProfilerActivity, profile
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    for s in steps[:2]:
        net.rnnTimeStep(s)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("style", list(STYLES))
def test_model_decodes_on_the_skinny_kernels(style):
    net, twin = _lm(style, "native"), _lm(style)
    twin.setParams(net.params().clone())
    x = torch.randint(0, V, (3, 9), generator=torch.Generator().manual_seed(1)).to(DEV)
    fallback.reset()
    for chunk in (x[:, :5], x[:, 5:6], x[:, 6:7]):
        got, want = net.rnnTimeStep(chunk)[0], twin.rnnTimeStep(chunk)[0]
        rel = ((got - want).norm() / want.norm()).item()
        print(f"{style} chunk of {chunk.shape[1]}: rel {rel:.3e}")
        assert rel < 3e-2
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    names = _step_kernels(net, x)
    # dense: 4 per block and the vocabulary projection; sparse: Wqkv, Wo and two grouped products per block
    dense, grouped = (9, 0) if style != "moe" else (5, 4)
    assert sum("skinny_gemm_kernel" in n for n in names) == dense
    assert sum("skinny_grouped_kernel" in n for n in names) == grouped
    assert not any("moe_gather_kernel" in n for n in names)
    extra = [n for n in names if _is_torch_kernel(n) and "bfloat16tofloat32_copy_kernel" not in n]
    assert not extra and sum(_is_torch_kernel(n) for n in names) <= 1, sorted(set(extra))
    # generation: graph replay gives the pinned run's bits
    prompt = x[:, :5].contiguous()
    pinned = net.generate(prompt, maxNewTokens=12, lengthPenalty=0.0, pinPositions=True)
    graph = net.generate(prompt, maxNewTokens=12, lengthPenalty=0.0, useGraph=True)
    assert torch.equal(graph.tokens, pinned.tokens) and torch.equal(graph.scores, pinned.scores)
    assert net.lastGenerationStats["graphReplays"] > 0
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    # nothing is derived from the parameters, so nothing can go stale
    fresh = _lm(style, "native", seed=11)
    net.rnnClearPreviousState()
    net.setParams(fresh.params().clone())
    assert torch.equal(net.rnnTimeStep(prompt)[0], fresh.rnnTimeStep(prompt)[0])
    # back at the default the step's launch list is that of a network that never had a format
    net.rnnClearPreviousState()
    net.rnnSetWeightDataType(None)
    plain = _step_kernels(net, x)
    assert plain == _step_kernels(twin, x) and not any("skinny_" in n for n in plain)
