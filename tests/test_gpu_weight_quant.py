"""Weight-only MXFP8 / MXFP4 decoding on the GPU (csrc/gemm_wq.hip): the quantise and dequantise kernels bit for bit
against the torch reference, the skinny GEMM against an fp64 product of the same (exactly dequantised) operands with
the error measure and bound of tests/test_gpu_gemm.py, and a two-block language model decoding with quantised
weights against its twin that holds the dequantised values on the 16-bit path."""
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


def _tol(dt, K):
    """tests/test_gpu_gemm.py's bound for 16-bit operands."""
    return (2e-2 if dt == torch.bfloat16 else 4e-3) * max(1.0, (K / 64) ** 0.5)


@functools.lru_cache(maxsize=None)
def _weights(dt, K, N):
    """W [K, N] on the CPU, never modified: randn with an all-zero group, a tiny one and a large one."""
    w = torch.randn(K, N, generator=torch.Generator().manual_seed(K + N)) * 0.05
    w[:32, 0] = 0.0
    w[:32, 1] *= 2.0 ** -9
    w[:32, 2] *= 2.0 ** 7
    return w.to(dt)


@functools.lru_cache(maxsize=None)
def _packed(fmt, dt, K, N):
    """(QuantWeight on the CPU from the reference, its values in fp64)."""
    qw = TN.wq_quantize_reference(_weights(dt, K, N), fmt)
    return qw, TN.wq_dequantize_reference(qw, torch.float64)


def _on_gpu(qw):
    return TN.QuantWeight(qw.fmt, qw.K, qw.N, qw.codes.to(DEV), qw.scales.to(DEV))


@pytest.mark.parametrize("K,N", [(32, 16), (96, 77), (768, 80)])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_quantize_and_dequantize_are_the_references_bytes(fmt, dt, K, N):
    want, _ = _packed(fmt, dt, K, N)
    fallback.reset()
    got = TN.wq_quantize(_weights(dt, K, N).to(DEV), fmt)
    assert torch.equal(got.codes.cpu(), want.codes) and torch.equal(got.scales.cpu(), want.scales)
    strided = _weights(dt, K, N).t().contiguous().to(DEV).t()                     # K-contiguous source
    got_t = TN.wq_quantize(strided, fmt)
    assert torch.equal(got_t.codes.cpu(), want.codes) and torch.equal(got_t.scales.cpu(), want.scales)
    deq = TN.wq_dequant(got, dt)
    assert torch.equal(deq.cpu(), TN.wq_dequantize_reference(want, dt))
    assert fallback.count() == 0, fallback.summary()


@pytest.mark.parametrize("M,beta,act", [(1, 0.0, None), (3, 1.0, None), (16, 0.0, "gelu"), (17, 1.0, "gelu"),
                                        (64, 0.0, None), (65, 1.0, "gelu")])
@pytest.mark.parametrize("K,N", [(32, 16), (96, 77), (768, 2304), (3072, 80)])
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_skinny_gemm_against_fp64(fmt, dt, K, N, M, beta, act):
    """One group, an odd group count, a split-K shape, a ragged last column block with masked columns; M = 65 takes
    the dequantise + mmul path. Since dequantisation is exact, this compares what a 16-bit product compares."""
    qw, w64 = _packed(fmt, dt, K, N)
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(dt)
    bias = torch.randn(N, generator=g) if M != 16 else torch.randn(N, generator=g).to(dt)    # fp32 master or 16-bit
    c0 = torch.randn(M, N, generator=g).to(dt)
    ref = x.double() @ w64 + bias.double() + beta * c0.double()
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    sentinel = float("nan")
    runs = []
    for _ in range(2):
        buf = torch.full((M + 2, N + 5), sentinel, dtype=dt, device=DEV)           # rows after M, columns after N
        out = buf[:M, :N]
        if beta:
            out.copy_(c0)
        fallback.reset()
        r = TN.wq_linear(x.to(DEV), _on_gpu(qw), bias.to(DEV), act, out, beta)
        assert r is out and fallback.count() == 0, fallback.summary()
        host = buf.cpu()
        assert host[M:].isnan().all() and host[:, N:].isnan().all(), "nothing outside [M, N] changes"
        runs.append(host[:M, :N])
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), "two runs give the same bits"
    err = (runs[0].double() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    print(f"{fmt} {dt} M={M} K={K} N={N}: max err {err:.3e}, bound {_tol(dt, K) * scale:.3e}")
    assert err <= _tol(dt, K) * scale


V = 77
STYLES = {"bert": {}, "llama": dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu",
                                    positionEncoding="rotary")}


def _lm(style, fmt=None, seed=5):
    return TextGenerationTransformer(numLabels=V, hidden=128, layers=2, heads=2, inputShape=[16], maxPositions=96,
                                     seed=seed, dataType=DataType.BFLOAT16, weightDataType=fmt,
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
@pytest.mark.parametrize("fmt", FMTS)
def test_model_decodes_with_quantised_weights(fmt, style):
    net, twin = _lm(style, fmt), _lm(style)
    twin.setParams(net.params().clone())
    for name, l in net.layers_by_name.items():
        for k in l.wqKeys():
            qw = TN.wq_quantize_reference(l.W(k), fmt)
            twin.layers_by_name[name].setParam(k, TN.wq_dequantize_reference(qw, torch.float32))
    x = torch.randint(0, V, (3, 9), generator=torch.Generator().manual_seed(1)).to(DEV)
    fallback.reset()
    # a cached step against the twin on the 16-bit path: the bound of tests/test_gpu_attention_decode.py
    for chunk in (x[:, :5], x[:, 5:6], x[:, 6:7]):
        got, want = net.rnnTimeStep(chunk)[0], twin.rnnTimeStep(chunk)[0]
        rel = ((got - want).norm() / want.norm()).item()
        print(f"{fmt} {style} chunk of {chunk.shape[1]}: rel {rel:.3e}")
        assert rel < 3e-2
    assert (net.output(x)[0][:, :, 6:7] - got).abs().max() > 0, "only rnnTimeStep reads the quantised copies"
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    names = _step_kernels(net, x)
    assert sum("wq_gemm_kernel" in n for n in names) == 9           # 4 per block and the vocabulary projection
    extra = [n for n in names if _is_torch_kernel(n) and "bfloat16tofloat32_copy_kernel" not in n]
    assert not extra and sum(_is_torch_kernel(n) for n in names) <= 1, sorted(set(extra))
    # generation: graph replay gives the pinned run's bits; the fp8 cache and ragged prompts run on the kernels
    prompt = x[:, :5].contiguous()
    pinned = net.generate(prompt, maxNewTokens=12, lengthPenalty=0.0, pinPositions=True)
    graph = net.generate(prompt, maxNewTokens=12, lengthPenalty=0.0, useGraph=True)
    assert torch.equal(graph.tokens, pinned.tokens) and torch.equal(graph.scores, pinned.scores)
    assert net.lastGenerationStats["graphReplays"] > 0
    ragged = net.generate(prompt[:2], promptLengths=[5, 3], maxNewTokens=12)
    alone = net.generate(prompt[1:2, :3].contiguous(), maxNewTokens=12)
    assert torch.equal(ragged.tokens[1:2], alone.tokens)
    net.rnnClearPreviousState()
    net.rnnSetCacheDataType("fp8")
    assert net.generate(prompt, maxNewTokens=12).tokens.shape == (3, 12)
    assert net.helperCountFail() == 0 and fallback.count() == 0, fallback.summary()
    # back at the default the step's launch list is that of a network that never had a format
    net.rnnClearPreviousState()
    net.rnnSetCacheDataType(None)
    net.rnnSetWeightDataType(None)
    plain = _step_kernels(net, x)
    assert plain == _step_kernels(twin, x) and not any("wq_" in n for n in plain)
