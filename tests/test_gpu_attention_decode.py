"""Cached decoding on the GPU (csrc/attention_decode.hip): the key/value append and the decode-attention kernel
against the fp32 reference on the whole sequence, the key splits (accuracy, bitwise reproducibility, default count),
refused operands, and the layers' rnnTimeStep on top of them (bf16 GPU against fp32 CPU, no fallback, no torch
compute kernel in a steady-state step)."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(2, 2, 64), (1, 3, 128)]
# a single key; the 64-key block edge from both sides; a ragged 16-query wave; a chunk crossing a wave; a chunk
# crossing a block (and a 64-query tile); a chunk ending on a block edge
POS_TN = [(0, 1), (62, 1), (63, 1), (64, 1), (128, 1), (60, 3), (50, 17), (10, 65), (191, 2)]


def _err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


@functools.lru_cache(maxsize=None)
def _case(dt, B, H, D, pos, Tn):
    """(qkv [B, pos+Tn, 3E] in dt on the CPU, oracle [B, Tn, E]): attention_reference in fp32 on the whole sequence
    built from the rounded inputs, causal, last Tn rows. Computed once per case and never modified."""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + D + 7 * pos + Tn)
    qkv = (torch.randn(B, pos + Tn, 3 * H * D, generator=g) * 0.8).to(dt)
    ref = TN.attention_reference(qkv.float(), H, None, True)[:, pos:].contiguous()
    return qkv, ref


def _tcap(L):
    return (L // 64 + 1) * 64 + 64          # the next multiple of 64 above L, plus 64


def _cache(qkv, H, pos, Tn):
    """NaN-filled cache holding the history (appended in two calls) and the new chunk; -> (new chunk, kv)."""
    B, L, E3 = qkv.shape
    q = qkv.to(DEV)
    kv = torch.full((B, _tcap(L), E3 // 3 * 2), float("nan"), dtype=qkv.dtype, device=DEV)
    h1 = pos // 2
    for a, b in ((0, h1), (h1, pos)):
        if b > a:
            assert TN.attn_kv_append(q[:, a:b].contiguous(), kv, H, a) is kv
    new = q[:, pos:].contiguous()
    assert TN.attn_kv_append(new, kv, H, pos) is kv
    return new, kv


@pytest.mark.parametrize("pos,Tn", POS_TN)
@pytest.mark.parametrize("B,H,D", SHAPES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_decode_matches_reference(dt, B, H, D, pos, Tn):
    qkv, ref = _case(dt, B, H, D, pos, Tn)
    new, kv = _cache(qkv, H, pos, Tn)
    out = TN.attn_decode(new, kv, H, pos)
    assert out is not None and out.dtype == dt and out.shape == (B, Tn, H * D)
    assert torch.isfinite(out).all(), "a row past the valid length reached the products"
    e = _err(out, ref)
    print(f"decode {dt} B={B} H={H} D={D} pos={pos} Tn={Tn}: err {e:.3e}")
    assert e < 2e-2
    assert torch.isnan(kv[:, pos + Tn:]).all() and torch.isfinite(kv[:, :pos + Tn]).all()


@pytest.mark.parametrize("Tn", [1, 17])
@pytest.mark.parametrize("B,H,D", SHAPES)
def test_decode_splits(B, H, D, Tn):
    pos, dt = 300, torch.bfloat16
    qkv, ref = _case(dt, B, H, D, pos, Tn)
    new, kv = _cache(qkv, H, pos, Tn)
    for splits in (1, 2, 3, 5, 64):                        # uneven ranges; more splits than the 5 key blocks
        a = TN.attn_decode(new, kv, H, pos, splits=splits)
        b = TN.attn_decode(new, kv, H, pos, splits=splits)
        assert torch.isfinite(a).all()
        e = _err(a, ref)
        print(f"splits={splits} B={B} H={H} D={D} Tn={Tn}: err {e:.3e}")
        assert e < 2e-2
        assert torch.equal(a, b), f"splits={splits} is not reproducible"
    default = TN.attn_decode_splits(B, Tn, H, D, pos + Tn)
    assert 1 <= default <= 5
    assert torch.equal(TN.attn_decode(new, kv, H, pos), TN.attn_decode(new, kv, H, pos, splits=default))


def test_default_splits_is_a_pure_function_of_the_shape():
    assert TN.attn_decode_splits(1, 1, 12, 64, 64) == 1                 # one key block: nothing to split
    assert TN.attn_decode_splits(128, 1, 12, 64, 4096) == 1             # 1536 blocks fill the device by themselves
    for L in (65, 128, 1000, 4096, 100000):
        s = TN.attn_decode_splits(1, 1, 12, 64, L)
        assert 1 <= s <= (L + 63) // 64                                 # never more splits than key blocks
        assert s == TN.attn_decode_splits(1, 1, 12, 64, L)
    assert TN.attn_decode_splits(1, 1, 12, 64, 4096) > 1                # 12 blocks on 256 compute units: split


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_kv_append(dt):
    B, H, D, Tcap, pos, Tn = 2, 3, 64, 128, 37, 5
    E = H * D
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, Tn, 3 * E, generator=g).to(dt).to(DEV)
    before = torch.randn(B, Tcap, 2 * E, generator=g).to(dt).to(DEV)
    kv = before.clone()
    assert TN.attn_kv_append(qkv, kv, H, pos) is kv
    assert torch.equal(kv[:, pos:pos + Tn], qkv[:, :, E:])
    assert torch.equal(kv[:, :pos], before[:, :pos]) and torch.equal(kv[:, pos + Tn:], before[:, pos + Tn:])
    kv = before.clone()
    assert TN.attn_kv_append(qkv, kv, H, Tcap - Tn + 1) is None            # pos + Tn > Tcap: status -1
    assert torch.equal(kv, before)
    assert TN.attn_kv_append(qkv, kv, H, Tcap - Tn) is kv                  # the last rows of the cache
    assert torch.equal(kv[:, Tcap - Tn:], qkv[:, :, E:]) and torch.equal(kv[:, :Tcap - Tn], before[:, :Tcap - Tn])


def test_unsupported_operands_are_refused():
    B, H, Tn = 2, 2, 3
    for D, dt in ((32, torch.bfloat16), (64, torch.float32)):
        E = H * D
        qkv = torch.randn(B, Tn, 3 * E, device=DEV).to(dt)
        kv = torch.zeros(B, 64, 2 * E, device=DEV, dtype=dt)
        assert not TN.attn_decode_supported(qkv, kv, H)
        assert TN.attn_kv_append(qkv, kv, H, 0) is None
        assert TN.attn_decode(qkv, kv, H, 0) is None
        assert torch.count_nonzero(kv) == 0


def _sa_net(dt, device, nOut):
    b = (NeuralNetConfiguration.Builder().seed(11).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0, 0.05)).list())
    b.layer(0, SelfAttentionLayer.Builder().nIn(128).nOut(nOut).nHeads(2).causal(True)
            .activation(Activation.IDENTITY).build())
    b.layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).nIn(nOut).nOut(5).activation(Activation.SOFTMAX).build())
    net = MultiLayerNetwork(b.build())
    net.init(device=device)
    return net


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.cpu())
    dst._params_changed()


def test_layer_with_unsupported_head_size_takes_the_reference_path():
    from deeplearning4j_amd.ops import fallback
    gpu = _sa_net(DataType.BFLOAT16, DEV, 64)                          # head size 32: outside the kernel
    cpu = _sa_net(DataType.FLOAT, torch.device("cpu"), 64)
    _copy_params(cpu, gpu)
    x = torch.randn(2, 128, 5, generator=torch.Generator().manual_seed(3))
    ref = cpu.output(x)
    fallback.reset()
    gpu.rnnClearPreviousState()
    got = torch.cat([gpu.rnnTimeStep(x[:, :, t:t + 1].to(DEV)) for t in range(5)], 2).cpu()
    assert fallback.count("attention") == 5
    rel = (got - ref).norm() / ref.norm()
    assert rel < 3e-2, rel


def _lm_graph(dt, device, T, V=11, E=128, H=2, F=24):
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.05)).graphBuilder())
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(T + 2).inputLength(T).build(), "tokens")
    g.addLayer("enc0", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True).build(),
               "emb")
    g.addLayer("enc1", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True).build(),
               "enc0")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V)
               .build(), "enc1")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device=device)
    return net


def test_network_time_step_matches_fp32_cpu():
    """bf16 rnnTimeStep on the kernels, token by token over T = 70 (past the first 64-key block and one cache
    growth), against the same weights in fp32 on the CPU; compared as tests/test_gpu_self_attention.py compares its
    GPU and CPU results (relative L2 error below 3e-2)."""
    T, MB, V = 70, 3, 11
    gpu = _lm_graph(DataType.BFLOAT16, DEV, T)
    cpu = _lm_graph(DataType.FLOAT, torch.device("cpu"), T)
    _copy_params(cpu, gpu)
    x = torch.randint(0, V, (MB, T), generator=torch.Generator().manual_seed(0))
    cpu.rnnClearPreviousState()
    ref = torch.cat([cpu.rnnTimeStep(x[:, t:t + 1])[0] for t in range(T)], 2)
    assert (ref - cpu.output(x)[0]).abs().max() < 1e-4
    from deeplearning4j_amd.ops import fallback
    fallback.reset()
    gpu.rnnClearPreviousState()
    xd = x.to(DEV)
    got = torch.cat([gpu.rnnTimeStep(xd[:, t:t + 1])[0] for t in range(T)], 2).cpu()
    torch.cuda.synchronize()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    assert torch.isfinite(got).all()
    rel = (got - ref).norm() / ref.norm()
    print(f"rnnTimeStep bf16 GPU vs fp32 CPU over T={T}: rel {rel:.3e}")
    assert rel < 3e-2, rel
    assert gpu.rnnGetPreviousState("enc1")["kv"].shape == (MB, T, 256)
    # a prompt of >= 64 tokens into an empty cache, then single steps: the same sequence again
    gpu.rnnClearPreviousState()
    got2 = torch.cat([gpu.rnnTimeStep(xd[:, :66])[0]] + [gpu.rnnTimeStep(xd[:, t:t + 1])[0] for t in range(66, T)],
                     2).cpu()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    rel2 = (got2 - ref).norm() / ref.norm()
    assert rel2 < 3e-2, rel2


def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


# The network API returns fp32: rnnTimeStep ends with ``.float()`` of the bf16 output layer's [mb, V, 1]
# activations, one torch conversion launch outside every layer (output() has the same one). It is the only torch
# kernel allowed in a decode step, and at most once.
_ALLOWED = ("bfloat16tofloat32_copy_kernel",)


def test_decode_step_launches_no_torch_compute_kernels():
    from torch.profiler import ProfilerActivity, profile
    from deeplearning4j_amd.models import TextGenerationTransformer
    net = TextGenerationTransformer(numLabels=77, inputShape=[64], hidden=128, layers=2, heads=2, maxPositions=64,
                                    dataType=DataType.BFLOAT16).init(device=DEV)
    x = torch.randint(0, 77, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    net.rnnTimeStep(steps[0])                                  # warm-up: kernel choices, cache allocation
    net.rnnTimeStep(steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 10, names
    for n in names:
        print("  kernel:", n[:120])
    assert sum("attn_decode_kernel" in n for n in names) == 2 and sum("attn_kv_append" in n for n in names) == 2
    assert sum("softmax_rows_kernel" in n for n in names) == 1         # the output layer's softmax is in-tree too
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    for n in sorted(set(torch_ks)):
        print("  torch:", n[:160])
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
