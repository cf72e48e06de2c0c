"""Grouped-query attention on the GPU (csrc/attention.hip, csrc/attention_decode.hip): H = 4 query heads over
Hkv in {1, 2} key/value heads, bf16 and fp16, head size 64 and 128.

``expand(qkv)`` is the multi-head projection with every K / V head repeated G = H / Hkv times. The forward, dQ and
the decode kernel must give the BITS the multi-head kernels give on the expanded operands (the same per-lane
arithmetic on the same values), and stay within the project's bound of the fp32 reference (error measure and 2e-2 of
tests/test_gpu_attention_decode.py). dK / dV are sums over a group the multi-head kernel does not form, so they are
compared with the fp32 explicit backward. Then a two-block GQA language model: a training step and generation against
fp32 on the CPU, pinned and graph-replayed generation, no fallback, no torch compute kernel in a decode step."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import fallback, nn_misc
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
B, H = 2, 4
DTS = [torch.bfloat16, torch.float16]
TOL = 2e-2
SEED = 0x5DEECE66D


def _err(a, b):
    """The error measure of tests/test_gpu_attention_decode.py."""
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def _stream(offset=1):
    st = nn_misc.PhiloxStream(DEV)
    st.seed = SEED
    st.offset.fill_(offset)
    return st


@functools.lru_cache(maxsize=None)
def _flash_case(dt, D, Hkv, T):
    """(qkv [B, T, E + 2*Ekv], dout [B, T, E], key-padding mask [B, T]) on the CPU, never modified."""
    g = torch.Generator().manual_seed(1000 * D + 10 * T + Hkv)
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)
    dout = torch.randn(B, T, H * D, generator=g).to(dt)
    lens = torch.tensor([T, max(1, T // 2)])
    mask = (torch.arange(T).reshape(1, T) < lens.reshape(B, 1)).float()
    return qkv, dout, mask


# (name, causal, masked, dropout)
MODES = [("plain", False, False, 0.0), ("causal", True, False, 0.0), ("mask", False, True, 0.0),
         ("causal+dropout", True, False, 0.25), ("dropout", False, False, 0.25)]


def _keep(T, drop):
    """The dropout mask the kernels draw at offset 1, scaled by 1 / keep_eff: [B, H, T, T] fp32 on the CPU."""
    _, keep_eff = TN.attn_drop_threshold(drop)
    return TN.attn_drop_mask(_stream(), B, H, T, drop).cpu().float() / keep_eff


# ------------------------------------------------------------------------------------------------ forward / backward
@pytest.mark.parametrize("T", [1, 63, 65, 130])
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_forward_and_backward(dt, D, Hkv, T):
    qkv, dout, mask = _flash_case(dt, D, Hkv, T)
    E, Ekv = H * D, Hkv * D
    qd, dd = qkv.to(DEV), dout.to(DEV)
    big = TN.gqa_expand(qd, H, Hkv).contiguous()
    assert TN.attn_supported(qd, H, Hkv) and big.shape[2] == 3 * E
    for name, causal, masked, drop in MODES:
        md = mask.to(DEV) if masked else None
        kw = dict(dropout=drop, rng=_stream()) if drop else {}
        out, lse = TN.attn_fwd(qd, H, md, causal, Hkv=Hkv, **kw)
        out_b, lse_b = TN.attn_fwd(big, H, md, causal, **kw)
        assert out.shape == (B, T, E) and lse.shape == (B, H, T)
        assert torch.equal(out, out_b), (name, "out differs from the multi-head kernel on expand(qkv)")
        assert torch.equal(lse, lse_b), (name, "lse")
        keep = _keep(T, drop) if drop else None
        m = mask if masked else None
        ref = TN.attention_reference(qkv.float(), H, m, causal, keep=keep, Hkv=Hkv)
        e = _err(out, ref)
        print(f"{name}: fwd {e:.3e}")
        assert e < TOL, (name, e)
        # backward: dQ is the multi-head kernel's, dK / dV the fp32 sums over each group; every column written
        dq_b = TN.attn_bwd(big, out_b, lse_b, dd, H, md, causal, **kw)[..., :E]
        buf = torch.full_like(qd, float("nan"))
        dqkv = TN.attn_bwd(qd, out, lse, dd, H, md, causal, Hkv=Hkv, dqkv=buf, **kw)
        assert dqkv is buf and dqkv.shape == qd.shape
        assert torch.isfinite(dqkv).all(), (name, "a column of dqkv was left unwritten")
        assert torch.equal(dqkv[..., :E], dq_b), (name, "dQ differs from the multi-head kernel on expand(qkv)")
        again = TN.attn_bwd(qd, out, lse, dd, H, md, causal, Hkv=Hkv, dqkv=torch.full_like(qd, float("nan")), **kw)
        assert torch.equal(again, dqkv), (name, "two runs differ")
        _, ctx = TN.attention_fwd_explicit(qkv.float(), H, m, causal, keep=keep, Hkv=Hkv)
        want = TN.attention_bwd_explicit(ctx, dout.float(), torch.float32)
        for what, sl in (("dQ", slice(0, E)), ("dK", slice(E, E + Ekv)), ("dV", slice(E + Ekv, E + 2 * Ekv))):
            e = _err(dqkv[..., sl], want[..., sl])
            print(f"{name}: {what} {e:.3e}")
            assert e < TOL, (name, what, e)


def test_the_entry_points_refuse_bad_head_counts():
    qkv = torch.zeros(1, 4, 6 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        TN.attn_fwd(qkv, 4, Hkv=3)
    lib = TN._lib()
    out = torch.zeros(1, 4, 256, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(1, 4, 4, device=DEV)
    args = lambda hkv, q=qkv: (1, TN._ptr(q), None, TN._ptr(out), TN._ptr(lse), 1, 4, 4, hkv, 64, 0.125, 0,  # noqa: E731
                               TN._stream())
    assert lib.dl4j_attn_fwd_gqa_dt(*args(0)) == -1 and lib.dl4j_attn_fwd_gqa_dt(*args(3)) == -1
    assert lib.dl4j_attn_fwd_gqa_dt(*args(1)) == 0
    assert lib.dl4j_attn_fwd_gqa_dt(*args(1, qkv.reshape(-1)[4:])) == -1         # misaligned
    assert lib.dl4j_attn_decode_splits_gqa(2, 1, 4, 3, 64, 100) == 1
    assert lib.dl4j_attn_decode_ws_bytes_gqa(2, 1, 4, 3, 64, 4) == 0
    assert lib.dl4j_attn_decode_ws_bytes_gqa(2, 1, 4, 1, 64, 4) == lib.dl4j_attn_decode_ws_bytes(2, 1, 4, 64, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ cache
POSITIONS = [0, 63, 64, 191]
RAGGED = {0: 0, 63: 10, 64: 1, 191: 63}                   # the upper bound -> where the second row stands
TCAP = 256


@functools.lru_cache(maxsize=None)
def _decode_case(dt, D, Hkv, Tn, pos, ragged):
    """History K | V [B, pos, 2*Ekv] and the new chunk [B, Tn, E + 2*Ekv] on the CPU, the rows' own positions."""
    g = torch.Generator().manual_seed(100000 * D + 1000 * pos + 10 * Tn + Hkv)
    hist = (torch.randn(B, pos, 2 * Hkv * D, generator=g) * 0.8).to(dt)
    new = (torch.randn(B, Tn, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)
    poss = (pos, RAGGED[pos]) if ragged else (pos, pos)
    return hist, new, poss


def _cache16(dt, D, Hkv, hist, poss):
    """NaN-filled 16-bit cache with every row's own history."""
    kv = torch.full((B, TCAP, 2 * Hkv * D), float("nan"), dtype=dt, device=DEV)
    for b, p in enumerate(poss):
        kv[b, :p] = hist[b, :p].to(DEV)
    return kv


def _short(pos, poss):
    return torch.tensor([pos - p for p in poss], dtype=torch.int32, device=DEV)


def _expand_cache(kv, Hkv, D):
    G = H // Hkv
    k, v = kv.reshape(B, TCAP, 2, Hkv, D).unbind(2)
    return torch.cat([k.repeat_interleave(G, dim=2).reshape(B, TCAP, -1),
                      v.repeat_interleave(G, dim=2).reshape(B, TCAP, -1)], dim=2).contiguous()


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_append(dt, D, Hkv, ragged):
    E, Ekv = H * D, Hkv * D
    for pos in POSITIONS:
        for Tn in (1, 17):
            hist, new, poss = _decode_case(dt, D, Hkv, Tn, pos, ragged)
            short = _short(pos, poss) if ragged else None
            nd = new.to(DEV)
            kv = _cache16(dt, D, Hkv, hist, poss)
            before = kv.clone()
            assert TN.attn_kv_append(nd, kv, H, pos, short, Hkv=Hkv) is kv
            R = TN.kv_fp8_row_bytes(H, D, Hkv)
            kv8 = torch.full((B, TCAP, R), 0xA5, dtype=torch.uint8, device=DEV)
            before8 = kv8.clone()
            assert TN.attn_kv_append(nd, kv8, H, pos, short, Hkv=Hkv) is kv8
            want8 = TN.kv_fp8_quantize_reference(nd[:, :, E:], Hkv)
            assert want8.shape == (B, Tn, R)
            for b, p in enumerate(poss):
                assert torch.equal(kv[b, p:p + Tn], nd[b, :, E:]), (pos, Tn, b)
                assert torch.equal(kv8[b, p:p + Tn], want8[b]), (pos, Tn, b, "fp8 rows")
                before[b, p:p + Tn] = kv[b, p:p + Tn]
                before8[b, p:p + Tn] = kv8[b, p:p + Tn]
            # nothing else changed (NaN compares as its bits)
            assert torch.equal(kv.view(torch.int16), before.view(torch.int16)), (pos, Tn)
            assert torch.equal(kv8, before8), (pos, Tn)
            deq = TN.kv_fp8_dequantize_reference(want8, H, D, dt, Hkv=Hkv)
            assert deq.shape == (B, Tn, 2 * Ekv) and _err(deq, nd[:, :, E:]) <= 2 ** -4   # 3 mantissa bits


@pytest.mark.parametrize("Tn", [1, 3, 17])
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_decode(dt, D, Hkv, Tn):
    """Tn*G slots: 2 .. 4 (one slot group inside a wave), 6 .. 12, 34 (a chunk crossing a 16-slot wave), 68 (crossing
    the 64-slot tile)."""
    E, Ekv = H * D, Hkv * D
    for ragged in (False, True):
        for pos in POSITIONS:
            hist, new, poss = _decode_case(dt, D, Hkv, Tn, pos, ragged)
            short = _short(pos, poss) if ragged else None
            nd = new.to(DEV)
            kv = _cache16(dt, D, Hkv, hist, poss)                # unused rows hold NaN
            assert TN.attn_kv_append(nd, kv, H, pos, short, Hkv=Hkv) is kv
            big_new, big_kv = TN.gqa_expand(nd, H, Hkv).contiguous(), _expand_cache(kv, Hkv, D)
            kv8 = torch.full((B, TCAP, TN.kv_fp8_row_bytes(Hkv, D)), 0xFF, dtype=torch.uint8, device=DEV)
            for b, p in enumerate(poss):
                kv8[b, :p] = TN.kv_fp8_quantize_reference(hist[b, :p].to(DEV), Hkv)
            assert TN.attn_kv_append(nd, kv8, H, pos, short, Hkv=Hkv) is kv8
            deq = torch.full_like(kv, float("nan"))
            for b, p in enumerate(poss):
                deq[b, :p + Tn] = TN.kv_fp8_dequantize_reference(kv8[b, :p + Tn], Hkv, D, dt)
            L = pos + Tn
            seen = kv[:, :L].cpu().float()
            ref = TN.attention_decode_reference(new[:, :, :E].float(), seen[:, :, :Ekv], seen[:, :, Ekv:], H, pos,
                                                short=None if short is None else short.cpu(), Hkv=Hkv)
            if not ragged:
                assert torch.isfinite(ref).all()
            for splits in (1, 3):
                tag = (ragged, pos, splits)
                out = TN.attn_decode(nd, kv, H, pos, splits=splits, short=short, Hkv=Hkv)
                assert out is not None and out.shape == (B, Tn, E)
                assert torch.isfinite(out).all(), tag
                mha = TN.attn_decode(big_new, big_kv, H, pos, splits=splits, short=short)
                assert torch.equal(out, mha), (tag, "differs from the multi-head kernel on the repeated cache")
                e = _err(out, ref)
                assert e < TOL, (tag, e)
                out8 = TN.attn_decode(nd, kv8, H, pos, splits=splits, short=short, Hkv=Hkv)
                assert torch.equal(out8, TN.attn_decode(nd, deq, H, pos, splits=splits, short=short, Hkv=Hkv)), \
                    (tag, "fp8 policy differs from the 16-bit kernel on the dequantised cache")
    assert TN.attn_decode_splits(32, 1, 12, 64, 4096, Hkv=4) == 16
    assert TN.attn_decode_splits(2048, 1, 12, 64, 4096, Hkv=1) == 1          # 2048 blocks fill the device


# ------------------------------------------------------------------------------------------------ network
V = 77


def _lm(dt, device, kv=2):
    return TextGenerationTransformer(numLabels=V, hidden=256, layers=2, heads=4, nKVHeads=kv, inputShape=[16],
                                     maxPositions=96, seed=5, dataType=dt).init(device=device)


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.to(dst.flattenedParams.device))
    dst._params_changed()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


def test_training_step_matches_fp32_cpu():
    """Compared as tests/test_gpu_self_attention.py compares its GPU and CPU gradients (relative L2 error < 3e-2)."""
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    assert tuple(gpu.layers_by_name["decoder_0"].params["Wqkv"].shape) == (256, 256 + 2 * 128)
    g = torch.Generator().manual_seed(3)
    T = 70
    x = torch.randint(0, V, (3, T), generator=g)
    y = torch.zeros(3, V, T)
    y.scatter_(1, torch.randint(0, V, (3, 1, T), generator=g), 1.0)
    fallback.reset()
    gpu.computeGradientAndScore([x.to(DEV)], [y.to(DEV)])
    torch.cuda.synchronize()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    cpu.computeGradientAndScore([x], [y])
    ga, gb = gpu.flattenedGradients.float().cpu(), cpu.flattenedGradients.float()
    rel = float((ga - gb).norm() / gb.norm())
    print(f"GQA training step bf16 GPU vs fp32 CPU: gradient rel {rel:.3e}, scores {gpu.score():.5f} {cpu.score():.5f}")
    assert rel < 3e-2, rel
    assert abs(gpu.score() - cpu.score()) < 3e-2 * abs(cpu.score())


def _loop_greedy(net, prompt, n):
    """The loop a user writes on rnnTimeStep (tests/test_gpu_generation.py): argmax of the fp32 output, fed back."""
    net.rnnClearPreviousState()
    out = net.rnnTimeStep(prompt)[0]
    toks, logp, dists = [], torch.zeros(out.shape[0], dtype=torch.float64), []
    for _ in range(n):
        p = out[:, :, -1]
        dists.append(p.float().cpu())
        t = p.argmax(1)
        logp += torch.log(p.double().gather(1, t[:, None]))[:, 0].cpu()
        toks.append(t)
        out = net.rnnTimeStep(t[:, None])[0]
    return torch.stack(toks, 1).cpu(), logp, dists


def test_generation_end_to_end():
    N = 24
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    prompt = torch.randint(0, V, (3, 5), generator=torch.Generator().manual_seed(2))
    want, logp, dists = _loop_greedy(gpu, prompt.to(DEV), N)
    fallback.reset()
    r = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert torch.equal(r.tokens.cpu(), want)
    assert (r.scores.cpu().double() - logp).abs().max() < 2e-5 * N
    st = gpu.rnnGetPreviousState("decoder_0")
    assert st["kv"].shape == (3, 5 + N - 1, 2 * 128)             # 2*Ekv columns: two key/value heads of 64
    # the fp32 CPU loop fed the same tokens: every step's distribution, compared as the layers are (rel L2 < 3e-2)
    cpu.rnnClearPreviousState()
    out = cpu.rnnTimeStep(prompt)[0]
    for i in range(N):
        assert _rel(dists[i], out[:, :, -1]) < 3e-2, i
        out = cpu.rnnTimeStep(want[:, i:i + 1])[0]
    # pinned positions and the replayed graph give the ordinary call's tokens
    pinned = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0, pinPositions=True)
    assert torch.equal(pinned.tokens, r.tokens)
    graph = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0, useGraph=True)
    stats = gpu.lastGenerationStats
    assert torch.equal(graph.tokens, pinned.tokens) and torch.equal(graph.scores, pinned.scores)
    assert stats["captures"] == 1 and stats["graphReplays"] > 0
    assert fallback.count() == 0, fallback.summary()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    # the fp8 cache of key/value heads: generation runs on the kernels too
    gpu.rnnClearPreviousState()
    gpu.rnnSetCacheDataType("fp8")
    r8 = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert r8.tokens.shape == r.tokens.shape and fallback.count() == 0, fallback.summary()
    assert gpu.rnnGetPreviousState("decoder_0")["kv"].shape == (3, 5 + N - 1, TN.kv_fp8_row_bytes(2, 64))


def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


# as in tests/test_gpu_attention_decode.py: rnnTimeStep ends with the fp32 conversion of the output layer's activations
_ALLOWED = ("bfloat16tofloat32_copy_kernel",)


def test_decode_step_launches_no_torch_compute_kernels():
    from torch.profiler import ProfilerActivity, profile
    net = _lm(DataType.BFLOAT16, DEV)
    x = torch.randint(0, V, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    net.rnnTimeStep(steps[0])
    net.rnnTimeStep(steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 10, names
    assert sum("attn_decode_gqa_kernel" in n for n in names) == 2 and sum("attn_kv_append" in n for n in names) == 2
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks


def test_flash_attention_autograd_function_takes_kv_heads():
    qkv, dout, _ = _flash_case(torch.bfloat16, 64, 2, 65)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    leaf = qd.clone().requires_grad_(True)
    out = TN.FlashAttention.apply(leaf, H, None, True, 0.0, None, 2)
    out.backward(dd)
    want, lse = TN.attn_fwd(qd, H, None, True, Hkv=2)
    assert torch.equal(out, want)
    assert torch.equal(leaf.grad, TN.attn_bwd(qd, want, lse, dd, H, None, True, Hkv=2))
