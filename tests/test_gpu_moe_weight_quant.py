"""Quantised mixture-of-experts experts on the GPU (dl4j_wq_gemm_grouped of csrc/gemm_wq.hip): the grouped skinny
product in both row-source modes against an fp64 product of the same (exactly dequantised) operands with the bound of
tests/test_gpu_weight_quant.py, and a two-block sparse language model decoding on quantised experts against its twin
that holds the dequantised experts on the 16-bit path."""
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
FMTS = ["fp8", "fp4"]
X, TOPK = 4, 2


def _tol(dt, K):
    """tests/test_gpu_weight_quant.py's bound for 16-bit operands."""
    return (2e-2 if dt == torch.bfloat16 else 4e-3) * max(1.0, (K / 64) ** 0.5)


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


@functools.lru_cache(maxsize=None)
def _experts(fmt, dt, K, N):
    """(QuantExperts on the CPU from the reference, every expert quantised on its own; their values in fp64)."""
    w = (torch.randn(X, K, N, generator=torch.Generator().manual_seed(K + N)) * 0.05).to(dt)
    qs = [TN.wq_quantize_reference(w[e], fmt) for e in range(X)]
    qe = TN.QuantExperts(fmt, X, K, N, torch.stack([q.codes for q in qs]), torch.stack([q.scales for q in qs]))
    return qe, torch.stack([TN.wq_dequantize_reference(q, torch.float64) for q in qs])


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "sorted"])
@pytest.mark.parametrize("Ntok", [1, 17, 64])
@pytest.mark.parametrize("K,N", [(32, 16), (96, 77), (1024, 48)])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_skinny_gemm_against_fp64(fmt, dt, K, N, Ntok, gather):
    """The gathered product carries the GELU epilogue (W1), the sorted one none (W2); the sorted input holds NaN in
    every row that no assignment owns: pad rows enter as zeros."""
    qe, w64 = _experts(fmt, dt, K, N)
    plan = _plan(Ntok)
    if K == 1024:
        assert TN._lib().dl4j_wq_gemm_grouped_workspace(qe.bits, Ntok, TOPK, X, N, K) > 0
    g = torch.Generator().manual_seed(Ntok + K)
    bias = torch.randn(X, N, generator=g)
    src = plan.src_of.long()
    live = src >= 0
    rows_x = torch.randn(Ntok, K, generator=g).to(dt)
    a = rows_x[src.clamp_min(0) // TOPK]                                     # the row every sorted row multiplies
    x = rows_x if gather else torch.where(live.unsqueeze(1), a, torch.full_like(a, float("nan")))
    ref = torch.zeros(plan.rows, N, dtype=torch.float64)
    for e in range(X):
        seg = slice(int(plan.off[e]), int(plan.off[e]) + int(plan.cnt[e]))
        ref[seg] = a[seg].double() @ w64[e] + bias[e].double()
    if gather:
        ref = torch.nn.functional.gelu(ref)
    gpu_plan = plan._replace(**{f: getattr(plan, f).to(DEV) for f in ("cnt", "off", "src_of")})
    gpu_qe = TN.QuantExperts(fmt, X, K, N, qe.codes.to(DEV), qe.scales.to(DEV))
    runs = []
    for _ in range(2):
        buf = torch.full((plan.rows + 2, N + 5), float("nan"), dtype=dt, device=DEV)
        out = buf[:plan.rows, :N]
        fallback.reset()
        r = TN.wq_gemm_grouped(x.to(DEV), gpu_qe, bias.to(DEV), gpu_plan, gather, "gelu" if gather else None, out)
        assert r is out and fallback.count() == 0, fallback.summary()
        host = buf.cpu()
        assert host[plan.rows:].isnan().all() and host[:, N:].isnan().all(), "nothing outside [Rcap, N] changes"
        assert host[:plan.rows][~live].isnan().all(), "pad rows and idle experts' segments are never written"
        runs.append(host[:plan.rows, :N][live])
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), "two runs give the same bits"
    err = (runs[0].double() - ref[live]).abs().max().item()
    scale = ref[live].abs().max().item() + 1e-6
    print(f"{fmt} {dt} Ntok={Ntok} K={K} N={N} gather={gather}: max err {err:.3e}, bound {_tol(dt, K) * scale:.3e}")
    assert err <= _tol(dt, K) * scale


V = 77
STYLES = {"bert": {}, "llama": dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu",
                                    positionEncoding="rotary")}


def _lm(style, fmt=None):
    return TextGenerationTransformer(numLabels=V, hidden=128, layers=2, heads=2, inputShape=[16], maxPositions=96,
                                     seed=5, dataType=DataType.BFLOAT16, nExperts=X, nExpertsPerToken=TOPK,
                                     expertWeightDataType=fmt, **STYLES[style]).init(device=DEV)


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
@pytest.mark.parametrize("fmt", FMTS)
def test_model_decodes_with_quantised_experts(fmt, style):
    net, twin = _lm(style, fmt), _lm(style)
    for l in net.layers_by_name.values():       # four times the fresh experts, as tests/test_moe_weight_quant.py; the
        for k in l.wqExpertKeys():              # pre-norm model's bf16 residual add still rounds the two paths'
            l.setParam(k, l.params[k] * 4.0)    # difference away (rel 0), the post-norm model shows ~2e-3
    twin.setParams(net.params().clone())
    for name, l in net.layers_by_name.items():
        for k in l.wqExpertKeys():
            w = l.W(k).reshape(X, -1, l.W(k).shape[1])
            deq = [TN.wq_dequantize_reference(TN.wq_quantize_reference(w[e], fmt), torch.float32) for e in range(X)]
            twin.layers_by_name[name].setParam(k, torch.cat(deq))
    x = torch.randint(0, V, (3, 30), generator=torch.Generator().manual_seed(1)).to(DEV)
    fallback.reset()
    # 15 rows: the skinny kernel; 69 rows: dequantise + the grouped GEMM; two single steps
    for chunk in (x[:, :5], x[:, 5:28], x[:, 28:29], x[:, 29:30]):
        got, want = net.rnnTimeStep(chunk)[0], twin.rnnTimeStep(chunk)[0]
        rel = ((got - want).norm() / want.norm()).item()
        print(f"{fmt} {style} chunk of {chunk.shape[1]}: rel {rel:.3e}")
        assert rel < 3e-2
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    names = _step_kernels(net, x)
    assert sum("wq_gemm_grouped_kernel" in n for n in names) == 4           # two per sparse block
    assert not any("moe_gather_kernel" in n for n in names)
    extra = [n for n in names if _is_torch_kernel(n) and "bfloat16tofloat32_copy_kernel" not in n]
    assert not extra and sum(_is_torch_kernel(n) for n in names) <= 1, sorted(set(extra))
    prompt = x[:, :5].contiguous()
    pinned = net.generate(prompt, maxNewTokens=12, lengthPenalty=0.0, pinPositions=True)
    graph = net.generate(prompt, maxNewTokens=12, lengthPenalty=0.0, useGraph=True)
    assert torch.equal(graph.tokens, pinned.tokens) and torch.equal(graph.scores, pinned.scores)
    assert net.lastGenerationStats["graphReplays"] > 0
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    # back at the default the step's launch list is that of a network that never had a format
    net.rnnClearPreviousState()
    net.rnnSetWeightDataType(None)
    plain = _step_kernels(net, x)
    assert plain == _step_kernels(twin, x) and not any("wq_" in n for n in plain)
