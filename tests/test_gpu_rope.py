"""Rotary position embeddings on the GPU (csrc/attention_rope.hip): B = 2, H = 4 query heads over Hkv in {4, 2, 1}
key/value heads, head size 64 and 128, bf16 and fp16.

(a) the refusals of the entry points; (b) ``attn_rope`` against the fp64 reference, every element within one rounding
of the 16-bit type; (c) ``attn_rope_append`` (16-bit and fp8 cache, uniform and ragged) bitwise against ``attn_rope``
followed by ``attn_kv_append``; (d) ``attn_decode`` over the rotated cache; (e) a two-block rotary language model with
grouped heads: a training step and generation against fp32 on the CPU, pinned and graph-replayed generation, the fp8
cache, ragged prompts, and the kernels of one decode step."""
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
B, H = 2, 4
DTS = [torch.bfloat16, torch.float16]
HKVS = [4, 2, 1]
THETA = 10000.0
TOL = 2e-2
# unit roundoff and smallest subnormal of the two types
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}


def _err(a, b):
    """The error measure of tests/test_gpu_attention_decode.py."""
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


@functools.lru_cache(maxsize=None)
def _chunk(dt, D, Hkv, T):
    """qkv [B, T, (H + 2*Hkv)*D] on the CPU, never modified."""
    g = torch.Generator().manual_seed(1000 * D + 10 * T + Hkv)
    return (torch.randn(B, T, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)


def _pair_sums(x, Hkv, D):
    """|x[j]| + |x[j + D/2]| for every element of the Q | K columns of x (fp64) -> [B, T, (H + Hkv)*D]."""
    Bx, T, _ = x.shape
    a = x[..., :(H + Hkv) * D].abs().reshape(Bx, T, H + Hkv, 2, D // 2)
    return (a[..., 0, :] + a[..., 1, :]).unsqueeze(3).expand(Bx, T, H + Hkv, 2, D // 2).reshape(Bx, T, -1)


def _short(vals):
    return None if vals is None else torch.tensor(vals, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ (a) refusals
def test_the_entry_points_refuse():
    lib = TN._lib()
    D = 64
    qkv = torch.zeros(1, 4, 12 * D, dtype=torch.bfloat16, device=DEV)
    kv = torch.zeros(1, 64, 8 * D, dtype=torch.bfloat16, device=DEV)
    kv8 = torch.zeros(1, 64, TN.kv_fp8_row_bytes(4, D), dtype=torch.uint8, device=DEV)
    fr = TN.rope_inv_freq(D, THETA, DEV)
    p, s = TN._ptr, TN._stream()
    rope = lib.dl4j_attn_rope_dt
    assert rope(1, p(qkv), p(fr), None, 1, 4, 4, 4, D, 0, 0, s) == 0
    assert rope(1, p(qkv), p(fr), None, 1, 4, 4, 4, 32, 0, 0, s) == -1               # head size
    assert rope(0, p(qkv), p(fr), None, 1, 4, 4, 4, D, 0, 0, s) == -1                # dtype
    assert rope(1, p(qkv.reshape(-1)[4:]), p(fr), None, 1, 2, 4, 4, D, 0, 0, s) == -1    # misaligned operand
    assert rope(1, p(qkv), p(fr[1:]), None, 1, 4, 4, 4, D, 0, 0, s) == -1            # misaligned frequencies
    assert rope(1, p(qkv), None, None, 1, 4, 4, 4, D, 0, 0, s) == -1                 # null inv_freq
    assert rope(1, None, p(fr), None, 1, 4, 4, 4, D, 0, 0, s) == -1
    assert rope(1, p(qkv), p(fr), None, 1, 4, 4, 3, D, 0, 0, s) == -1                # Hkv does not divide H
    assert rope(1, p(qkv), p(fr), None, 1, 4, 4, 4, D, -1, 0, s) == -1
    for fn, cache in ((lib.dl4j_attn_rope_append_dt, kv), (lib.dl4j_attn_rope_append_fp8_dt, kv8)):
        assert fn(1, p(qkv), p(cache), p(fr), None, 1, 4, 4, 4, D, 60, 64, s) == 0
        assert fn(1, p(qkv), p(cache), p(fr), None, 1, 4, 4, 4, D, 61, 64, s) == -1  # pos + Tn > Tcap
        assert fn(1, p(qkv), p(cache), p(fr), None, 1, 4, 4, 4, D, 0, 48, s) == -1   # Tcap % 64
        assert fn(1, p(qkv), None, p(fr), None, 1, 4, 4, 4, D, 0, 64, s) == -1
        assert fn(1, p(qkv), p(cache), None, None, 1, 4, 4, 4, D, 0, 64, s) == -1
        assert fn(1, p(qkv), p(cache), p(fr), None, 1, 4, 4, 3, D, 0, 64, s) == -1
        assert fn(1, p(qkv), p(cache), p(fr), None, 1, 4, 4, 4, 32, 0, 64, s) == -1
    torch.cuda.synchronize()
    # the wrappers hand the refusal on as None and leave the operands alone
    odd = torch.ones(1, 4, 12 * 32, dtype=torch.bfloat16, device=DEV)
    assert TN.attn_rope(odd, 4, 0, THETA) is None and bool((odd == 1).all())
    assert TN.attn_rope_append(qkv, kv, 4, 61, THETA) is None


# ------------------------------------------------------------------------------------------------ (b) attn_rope
@pytest.mark.parametrize("Hkv", HKVS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_rope_against_the_fp64_reference(dt, D, Hkv):
    """Every element within ONE rounding of a value of magnitude at most |x[j]| + |x[j + D/2]|, plus 1 % for the fp32
    arithmetic: |out - ref| <= 1.01 u (|x[j]| + |x[j + D/2]|) + tiny. The reference forms the angle as the kernel
    must: the fp32 product of the fp32 position and the fp32 inv_freq (at p = 131000 an fp64 angle differs by 3.7e-3
    in the cosine). pos = 131000 needs the accurate sincosf: the hardware sine is off by far more than the bound."""
    u, tiny = U[dt], TINY[dt]
    n = (H + Hkv) * D
    worst = 0.0
    for T in (1, 5, 67):
        x = _chunk(dt, D, Hkv, T)
        x64 = x.double()
        bound = 1.01 * u * _pair_sums(x64, Hkv, D) + tiny
        W = x.shape[2]
        for pos in (0, 63, 131000):
            for sv in ((None,) if pos == 0 else (None, [0, 3])):
                tag = (T, pos, sv)
                short = _short(sv)
                # the operand is a slice of a larger buffer whose other bytes must not change
                buf = torch.full((B * T * W + 256,), 7.0, dtype=dt, device=DEV)
                q = buf[128:128 + B * T * W].view(B, T, W)
                q.copy_(x.to(DEV))
                assert TN.attn_rope(q, H, pos, THETA, short, Hkv=Hkv) is q
                got = q.cpu()
                assert bool((buf[:128] == 7).all()) and bool((buf[128 + B * T * W:] == 7).all()), tag
                positions = TN.rope_positions(B, T, pos, None if sv is None else torch.tensor(sv, dtype=torch.int32))
                ref = TN.rope_reference(x64, H, positions, THETA, Hkv=Hkv)
                assert torch.equal(got[..., n:], x[..., n:]), (tag, "V columns changed")
                err = (got[..., :n].double() - ref[..., :n]).abs()
                ratio = (err / bound).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, (tag, ratio)
                # two runs agree bitwise
                q2 = x.to(DEV)
                assert TN.attn_rope(q2, H, pos, THETA, short, Hkv=Hkv) is q2
                assert torch.equal(q2.cpu().view(torch.int16), got.view(torch.int16)), (tag, "two runs differ")
                # the inverse brings every element back within two such roundings
                assert TN.attn_rope(q2, H, pos, THETA, short, Hkv=Hkv, inverse=True) is q2
                back = q2.cpu()
                assert torch.equal(back[..., n:], x[..., n:]), tag
                r2 = ((back[..., :n].double() - x64[..., :n]).abs() / (2 * bound)).max().item()
                assert r2 <= 1.0, (tag, "inverse", r2)
                if pos:
                    assert not torch.equal(got[..., :n], x[..., :n]), tag
    print(f"attn_rope {dt} D={D} Hkv={Hkv}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ (c) fused append
TCAP = 256
APPEND_POS = {0: 0, 61: 7, 130: 66}                      # the upper bound -> where the second row stands when ragged


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("Hkv", HKVS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_rope_append_is_rope_then_append(dt, D, Hkv, ragged):
    R = TN.kv_fp8_row_bytes(H, D, Hkv)
    for Tn in (1, 3, 70):
        x = _chunk(dt, D, Hkv, Tn).to(DEV)
        for pos, second in APPEND_POS.items():
            tag = (Tn, pos)
            short = _short([0, pos - second]) if ragged else None
            rows = (pos, second) if ragged else (pos, pos)
            # the two existing calls on copies
            want_q = x.clone()
            assert TN.attn_rope(want_q, H, pos, THETA, short, Hkv=Hkv) is want_q
            for fp8 in (False, True):
                if fp8:
                    kv = torch.full((B, TCAP, R), 0xA5, dtype=torch.uint8, device=DEV)
                else:
                    kv = torch.full((B, TCAP, 2 * Hkv * D), float("nan"), dtype=dt, device=DEV)
                want_kv = kv.clone()
                assert TN.attn_kv_append(want_q, want_kv, H, pos, short, Hkv=Hkv) is want_kv
                q = x.clone()
                before = kv.clone()
                assert TN.attn_rope_append(q, kv, H, pos, THETA, short, Hkv=Hkv) is kv
                bits = (lambda t: t) if fp8 else (lambda t: t.view(torch.int16))      # NaN compares as its bits
                assert torch.equal(q.view(torch.int16), want_q.view(torch.int16)), (tag, fp8, "qkv")
                assert torch.equal(bits(kv), bits(want_kv)), (tag, fp8, "cache")
                for b, p in enumerate(rows):
                    assert not torch.equal(bits(kv[b, p:p + Tn]), bits(before[b, p:p + Tn])), (tag, fp8, b)
                    before[b, p:p + Tn] = kv[b, p:p + Tn]
                assert torch.equal(bits(kv), bits(before)), (tag, fp8, "a byte outside the new rows changed")


# ------------------------------------------------------------------------------------------------ (d) decode
@pytest.mark.parametrize("Tn", [1, 17])
@pytest.mark.parametrize("Hkv", HKVS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_decode_over_the_rotated_cache(dt, D, Hkv, Tn):
    pos = 191
    E, Ekv = H * D, Hkv * D
    g = torch.Generator().manual_seed(100 * D + 10 * Tn + Hkv)
    hist = (torch.randn(B, pos, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)        # the tokens before, unrotated
    new = (torch.randn(B, Tn, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)
    # the cache as the layer builds it: the prompt in one chunk, then the new chunk
    kv = torch.full((B, TCAP, 2 * Ekv), float("nan"), dtype=dt, device=DEV)
    assert TN.attn_rope_append(hist.to(DEV), kv, H, 0, THETA, Hkv=Hkv) is kv
    nd = new.to(DEV)
    assert TN.attn_rope_append(nd, kv, H, pos, THETA, Hkv=Hkv) is kv
    # fp32 reference on rope_reference-rotated operands
    rot = TN.rope_reference(torch.cat([hist, new], 1).float(), H, torch.arange(pos + Tn), THETA, Hkv=Hkv)
    ref = TN.attention_decode_reference(rot[:, pos:, :E], rot[:, :, E:E + Ekv], rot[:, :, E + Ekv:], H, pos, Hkv=Hkv)
    for splits in (1, 3):
        out = TN.attn_decode(nd, kv, H, pos, splits=splits, Hkv=Hkv)
        assert out is not None and torch.isfinite(out).all()
        e = _err(out, ref)
        assert e < TOL, (splits, e)


# ------------------------------------------------------------------------------------------------ (e) network
V = 77


def _lm(dt, device, rotary=True):
    return TextGenerationTransformer(numLabels=V, hidden=256, layers=2, heads=4, nKVHeads=2, inputShape=[16],
                                     maxPositions=96, seed=5, dataType=dt,
                                     positionEncoding="rotary" if rotary else None).init(device=device)


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.to(dst.flattenedParams.device))
    dst._params_changed()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


def test_training_step_matches_fp32_cpu():
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    assert "Wpos" not in gpu.layers_by_name["embeddings"].params
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
    print(f"rotary training step bf16 GPU vs fp32 CPU: gradient rel {rel:.3e}, scores {gpu.score():.5f} "
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


def test_generation_end_to_end():
    N = 24
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
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


def test_ragged_prompts_equal_every_row_alone():
    net = _lm(DataType.BFLOAT16, DEV)
    N, lens = 24, [5, 3]
    prompt = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(4)).to(DEV)
    fallback.reset()
    got = net.generate(prompt, promptLengths=lens, maxNewTokens=N)
    for b, n in enumerate(lens):
        alone = net.generate(prompt[b:b + 1, :n].contiguous(), maxNewTokens=N)
        assert torch.equal(got.tokens[b:b + 1], alone.tokens), f"row {b} ({n} tokens)"
    assert fallback.count() == 0, fallback.summary()


def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


# as in tests/test_gpu_attention_decode.py: rnnTimeStep ends with the fp32 conversion of the output layer's activations
_ALLOWED = ("bfloat16tofloat32_copy_kernel",)


def _step_kernels(net):
    from torch.profiler import ProfilerActivity, profile
    x = torch.randint(0, V, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    net.rnnTimeStep(steps[0])
    net.rnnTimeStep(steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_a_decode_step_gains_no_launch():
    names = _step_kernels(_lm(DataType.BFLOAT16, DEV))
    assert len(names) > 10, names
    assert sum("rope_append" in n for n in names) == 2 and sum("attn_kv_append" in n for n in names) == 0
    assert sum("attn_rope_kernel" in n for n in names) == 0
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
    learned = _step_kernels(_lm(DataType.BFLOAT16, DEV, rotary=False))
    assert sum("attn_kv_append" in n for n in learned) == 2
    assert len(names) == len(learned), (len(names), len(learned))
