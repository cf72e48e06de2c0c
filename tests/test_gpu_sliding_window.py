"""Sliding-window attention on the GPU (the WIN instances of csrc/attention_body.h and csrc/attention_decode.hip):
query p sees keys p - W < k <= p. B = 2, H = 4 query heads over Hkv in {4, 1} key/value heads, head size 64 and 128,
bf16 and fp16; the error measure and the 2e-2 bound of tests/test_gpu_attention_decode.py.

Flash forward / backward against the fp32 references, two runs bit for bit, W >= T against the unwindowed entry
points bit for bit, dropout under two windows explained by the one keep mask. Decode over a cache of up to 330 rows
(16-bit and fp8, uniform and ragged, 1 / 2 / 4 splits), W >= L against the unwindowed kernel bit for bit, a
block-aligned window against the unwindowed kernel on the sliced cache bit for bit, and NaN in every block before the
window changing nothing (skipped, not masked). Then a two-block Llama-style model with one windowed block."""
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
DROP = 0.25


def _err(a, b):
    """The error measure of tests/test_gpu_attention_decode.py."""
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _stream(offset=1):
    st = nn_misc.PhiloxStream(DEV)
    st.seed = SEED
    st.offset.fill_(offset)
    return st


# ------------------------------------------------------------------------------------------------ flash
WINDOWS = [1, 17, 64, 65, 129]
# (name, masked, dropout); every mode is causal
MODES = [("causal", False, 0.0), ("causal+mask", True, 0.0), ("causal+dropout", False, DROP)]


@functools.lru_cache(maxsize=None)
def _flash_case(dt, D, Hkv, T):
    """(qkv [B, T, E + 2*Ekv], dout [B, T, E], key-padding mask [B, T]) on the CPU, never modified."""
    g = torch.Generator().manual_seed(1000 * D + 10 * T + Hkv)
    qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)
    dout = torch.randn(B, T, H * D, generator=g).to(dt)
    lens = torch.tensor([T, max(1, T // 2)])
    mask = (torch.arange(T).reshape(1, T) < lens.reshape(B, 1)).float()
    return qkv, dout, mask


@functools.lru_cache(maxsize=None)
def _keep(T):
    """The dropout mask the kernels draw at offset 1, scaled by 1 / keep_eff: [B, H, T, T] fp32 on the CPU."""
    _, keep_eff = TN.attn_drop_threshold(DROP)
    return TN.attn_drop_mask(_stream(), B, H, T, DROP).cpu().float() / keep_eff


@pytest.mark.parametrize("T", [65, 130, 260])
@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_forward_and_backward(dt, D, Hkv, T):
    """T = 260 with W = 17: the last tile (q0 = 256) starts at key block 3, so the D = 64 forward, which stages two
    blocks per round, starts inside a round.

    W = 1 with dropout is the sharp case of the backward: a query sees itself only, P = 1, and the exact
    dS = D dP - Delta is zero, so dQ = dK = 0 and any error in Delta stands alone. The windowed dropout kernels take
    Delta from their own probabilities (csrc/attention_body.h); taken from the stored output O = V / keep_eff, which
    is rounded to 16 bits, the same case measured dK 2.15e-02 in bf16 at D = 128 with one kv head."""
    qkv, dout, mask = _flash_case(dt, D, Hkv, T)
    E, Ekv = H * D, Hkv * D
    qd, dd = qkv.to(DEV), dout.to(DEV)
    assert TN.attn_supported(qd, H, Hkv)
    for name, masked, drop in MODES:
        md = mask.to(DEV) if masked else None
        m = mask if masked else None
        kw = dict(dropout=drop, rng=_stream()) if drop else {}
        keep = _keep(T) if drop else None               # ONE mask for every window: skipped blocks do not shift it
        for W in WINDOWS:
            tag = (name, W)
            out, lse = TN.attn_fwd(qd, H, md, True, Hkv=Hkv, window=W, **kw)
            assert out.shape == (B, T, E) and lse.shape == (B, H, T)
            ref = TN.attention_reference(qkv.float(), H, m, True, keep=keep, Hkv=Hkv, window=W)
            e = _err(out, ref)
            print(f"{name} W={W}: fwd {e:.3e}")
            assert e < TOL, (tag, e)
            buf = torch.full_like(qd, float("nan"))
            dqkv = TN.attn_bwd(qd, out, lse, dd, H, md, True, Hkv=Hkv, dqkv=buf, window=W, **kw)
            assert dqkv is buf and torch.isfinite(dqkv).all(), (tag, "a column of dqkv was left unwritten")
            _, ctx = TN.attention_fwd_explicit(qkv.float(), H, m, True, keep=keep, Hkv=Hkv, window=W)
            want = TN.attention_bwd_explicit(ctx, dout.float(), torch.float32)
            for what, sl in (("dQ", slice(0, E)), ("dK", slice(E, E + Ekv)), ("dV", slice(E + Ekv, E + 2 * Ekv))):
                e = _err(dqkv[..., sl], want[..., sl])
                print(f"{name} W={W}: {what} {e:.3e}")
                assert e < TOL, (tag, what, e)
            out2, lse2 = TN.attn_fwd(qd, H, md, True, Hkv=Hkv, window=W, **kw)
            again = TN.attn_bwd(qd, out2, lse2, dd, H, md, True, Hkv=Hkv, dqkv=torch.full_like(qd, float("nan")),
                                window=W, **kw)
            assert torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(again, dqkv), (tag, "two runs")
        # a window that reaches the first key: the bits of the kernels without one
        out_u, lse_u = TN.attn_fwd(qd, H, md, True, Hkv=Hkv, **kw)
        dqkv_u = TN.attn_bwd(qd, out_u, lse_u, dd, H, md, True, Hkv=Hkv, **kw)
        for W in (T, T + 7):
            out, lse = TN.attn_fwd(qd, H, md, True, Hkv=Hkv, window=W, **kw)
            assert torch.equal(out, out_u) and torch.equal(lse, lse_u), (name, W, "forward bits")
            dqkv = TN.attn_bwd(qd, out, lse, dd, H, md, True, Hkv=Hkv, window=W, **kw)
            assert torch.equal(_bits(dqkv), _bits(dqkv_u)), (name, W, "backward bits")


def test_the_entry_points_refuse_a_bad_window():
    qkv = torch.zeros(1, 4, 3 * 4 * 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="window"):
        TN.attn_fwd(qkv, 4, None, True, window=0)
    with pytest.raises(ValueError, match="causal"):
        TN.attn_fwd(qkv, 4, None, False, window=3)
    lib = TN._lib()
    out = torch.zeros(1, 4, 256, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(1, 4, 4, device=DEV)
    args = lambda w: (1, TN._ptr(qkv), None, TN._ptr(out), TN._ptr(lse), 1, 4, 4, 4, 64, 0.125, w, 0.0, 0, None,  # noqa: E731
                      TN._stream())
    assert lib.dl4j_attn_fwd_win_dt(*args(0)) == -1 and lib.dl4j_attn_fwd_win_dt(*args(-3)) == -1
    assert lib.dl4j_attn_fwd_win_dt(*args(2)) == 0
    kv = torch.zeros(1, 64, 2 * 4 * 64, dtype=torch.bfloat16, device=DEV)
    dargs = lambda w: (1, TN._ptr(qkv), TN._ptr(kv), TN._ptr(out), None, None, 1, 4, 4, 4, 64, 10, 64, w, 1, 0.125,  # noqa: E731
                       TN._stream())
    assert lib.dl4j_attn_decode_win_dt(*dargs(0)) == -1 and lib.dl4j_attn_decode_win_dt(*dargs(5)) == 0
    torch.cuda.synchronize()


def test_flash_attention_autograd_function_takes_the_window():
    qkv, dout, _ = _flash_case(torch.bfloat16, 64, 1, 130)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    leaf = qd.clone().requires_grad_(True)
    out = TN.FlashAttention.apply(leaf, H, None, True, 0.0, None, 1, 17)
    out.backward(dd)
    want, lse = TN.attn_fwd(qd, H, None, True, Hkv=1, window=17)
    assert torch.equal(out, want)
    assert torch.equal(leaf.grad, TN.attn_bwd(qd, want, lse, dd, H, None, True, Hkv=1, window=17))


# ------------------------------------------------------------------------------------------------ decode
L_MAX, TCAP = 330, 384
ROW1 = 20                                                 # ragged: where the second row stands (shorter than W >= 64)
DEC_WINDOWS = [1, 64, 100, 129]
SPLITS = [1, 2, 4]


@functools.lru_cache(maxsize=None)
def _decode_case(dt, D, Hkv, Tn):
    """History K | V [B, pos, 2*Ekv] and the new chunk [B, Tn, E + 2*Ekv] on the CPU; pos + Tn = 330."""
    pos = L_MAX - Tn
    g = torch.Generator().manual_seed(100000 * D + 10 * Tn + Hkv)
    hist = (torch.randn(B, pos, 2 * Hkv * D, generator=g) * 0.8).to(dt)
    new = (torch.randn(B, Tn, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt)
    return hist, new, pos


def _caches(dt, D, Hkv, Tn, ragged):
    """(new chunk on the device, 16-bit cache, fp8 cache, its dequantised twin, pos, the rows' positions, shortfall):
    unused rows hold NaN / 0xFF, the new rows are appended."""
    hist, new, pos = _decode_case(dt, D, Hkv, Tn)
    poss = (pos, ROW1) if ragged else (pos, pos)
    short = torch.tensor([pos - p for p in poss], dtype=torch.int32, device=DEV) if ragged else None
    nd = new.to(DEV)
    kv = torch.full((B, TCAP, 2 * Hkv * D), float("nan"), dtype=dt, device=DEV)
    kv8 = torch.full((B, TCAP, TN.kv_fp8_row_bytes(Hkv, D)), 0xFF, dtype=torch.uint8, device=DEV)
    for b, p in enumerate(poss):
        kv[b, :p] = hist[b, :p].to(DEV)
        kv8[b, :p] = TN.kv_fp8_quantize_reference(hist[b, :p].to(DEV), Hkv)
    assert TN.attn_kv_append(nd, kv, H, pos, short, Hkv=Hkv) is kv
    assert TN.attn_kv_append(nd, kv8, H, pos, short, Hkv=Hkv) is kv8
    deq = torch.full_like(kv, float("nan"))
    for b, p in enumerate(poss):
        deq[b, :p + Tn] = TN.kv_fp8_dequantize_reference(kv8[b, :p + Tn], Hkv, D, dt)
    return nd, kv, kv8, deq, pos, poss, short


def _reference(new, cache, Hkv, D, pos, Tn, short, W):
    E, Ekv = H * D, Hkv * D
    seen = cache[:, :pos + Tn].cpu().float()
    return TN.attention_decode_reference(new[:, :, :E].float().cpu(), seen[:, :, :Ekv], seen[:, :, Ekv:], H, pos,
                                         short=None if short is None else short.cpu(), Hkv=Hkv, window=W)


@pytest.mark.parametrize("Tn", [1, 3, 70])
@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_decode(dt, D, Hkv, Tn):
    E = H * D
    for ragged in (False, True):
        nd, kv, kv8, deq, pos, poss, short = _caches(dt, D, Hkv, Tn, ragged)
        L = pos + Tn
        for W in DEC_WINDOWS:
            ref = _reference(nd, kv, Hkv, D, pos, Tn, short, W)
            ref8 = _reference(nd, deq, Hkv, D, pos, Tn, short, W)
            assert torch.isfinite(ref).all() and torch.isfinite(ref8).all()
            # every row of the blocks wholly before the row's window (of its first query) holds NaN in this copy
            holes = kv.clone()
            for b, p in enumerate(poss):
                holes[b, :max(0, p - W + 1) // 64 * 64] = float("nan")
            for splits in SPLITS:
                tag = (ragged, W, splits)
                out = TN.attn_decode(nd, kv, H, pos, splits=splits, short=short, Hkv=Hkv, window=W)
                assert out is not None and out.shape == (B, Tn, E) and torch.isfinite(out).all(), tag
                e = _err(out, ref)
                print(f"ragged={ragged} W={W} splits={splits}: {e:.3e}")
                assert e < TOL, (tag, e)
                again = TN.attn_decode(nd, holes, H, pos, splits=splits, short=short, Hkv=Hkv, window=W)
                assert torch.equal(again, out), (tag, "a block before the window was read")
                out8 = TN.attn_decode(nd, kv8, H, pos, splits=splits, short=short, Hkv=Hkv, window=W)
                e8 = _err(out8, ref8)
                assert e8 < TOL, (tag, "fp8", e8)
                assert torch.equal(out8, TN.attn_decode(nd, deq, H, pos, splits=splits, short=short, Hkv=Hkv,
                                                        window=W)), (tag, "fp8 policy vs the dequantised cache")
        # a window that reaches key 0: the bits of the kernel without one at the same split count
        for W in (L, L + 50):
            for splits in SPLITS:
                for cache in (kv, kv8):
                    assert torch.equal(TN.attn_decode(nd, cache, H, pos, splits=splits, short=short, Hkv=Hkv, window=W),
                                       TN.attn_decode(nd, cache, H, pos, splits=splits, short=short, Hkv=Hkv)), \
                        (ragged, W, splits, cache.dtype)


@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
def test_a_block_aligned_window_is_the_unwindowed_kernel_on_the_sliced_cache(dt, D, Hkv):
    """One query, one split, the window starting on a block boundary: the same blocks in the same order, every key of
    them visible, so the bits of the kernel without a window on kv[:, pos - W + 1:] at position W - 1."""
    nd, kv, kv8, _, pos, _, _ = _caches(dt, D, Hkv, 1, False)
    for W in (74, 138, 266):
        first = pos - W + 1
        assert first % 64 == 0 and first > 0
        for cache in (kv, kv8):
            got = TN.attn_decode(nd, cache, H, pos, splits=1, Hkv=Hkv, window=W)
            sliced = cache[:, first:].contiguous()
            assert sliced.shape[1] % 64 == 0
            want = TN.attn_decode(nd, sliced, H, W - 1, splits=1, Hkv=Hkv)
            assert want is not None and torch.equal(got, want), (W, cache.dtype)


def test_the_default_split_count_follows_the_keys_a_step_reads():
    # batch 1, 12 heads of 64: 4096 cached keys under a window of 256 are split as the 4 (here) or 5 key blocks the
    # window touches are, not as 64 blocks
    assert TN.attn_decode_splits(1, 1, 12, 64, 4096) == 16
    assert TN.attn_decode_splits(1, 1, 12, 64, 4096, window=256) == TN.attn_decode_splits(1, 1, 12, 64, 256) == 2
    assert TN.attn_decode_splits(1, 1, 12, 64, 4130, window=256) == TN.attn_decode_splits(1, 1, 12, 64, 290) == 2
    assert TN.attn_decode_splits(1, 1, 12, 64, 4096, window=5000) == 16
    assert TN.attn_decode_splits(1, 1, 12, 64, 4097, window=1) == 1
    assert TN.attn_decode_splits(1, 3, 12, 64, 100, Hkv=4, window=64) == TN.attn_decode_splits(1, 3, 12, 64, 100, Hkv=4)


# ------------------------------------------------------------------------------------------------ network
V = 77
WINDOW = 20


def _lm(dt, device, window=(WINDOW, None)):
    """Two Llama-style blocks (rotary, RMSNorm, SwiGLU, 4 query heads over 2 key/value heads of 64); the first has a
    window, the second attends over the whole prefix."""
    return TextGenerationTransformer(numLabels=V, hidden=256, layers=2, heads=4, nKVHeads=2, inputShape=[16],
                                     maxPositions=96, seed=5, dataType=dt, positionEncoding="rotary",
                                     normalization="rms", normPlacement="pre", ffnActivation="swiglu",
                                     attentionWindow=None if window is None else list(window)).init(device=device)


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.to(dst.flattenedParams.device))
    dst._params_changed()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


def test_training_step_matches_fp32_cpu():
    """The measure and bounds of tests/test_gpu_gqa.py / tests/test_gpu_llama_block.py for the same comparison:
    gradient rel L2 < 3e-2, score within 3e-2."""
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    assert gpu.layers_by_name["decoder_0"].conf.attentionWindow == WINDOW
    assert gpu.layers_by_name["decoder_1"].conf.attentionWindow is None
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
    print(f"windowed training step bf16 GPU vs fp32 CPU: gradient rel {rel:.3e}, scores {gpu.score():.5f} "
          f"{cpu.score():.5f}")
    assert rel < 3e-2, rel
    assert abs(gpu.score() - cpu.score()) < 3e-2 * abs(cpu.score())
    # the window is in the step: the same parameters without it give another score
    full = _lm(DataType.FLOAT, CPU, None)
    _copy_params(full, cpu)
    full.computeGradientAndScore([x], [y])
    assert abs(full.score() - cpu.score()) > 1e-6


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


@pytest.mark.parametrize("Tp", [30, 70], ids=["decode-prompt", "flash-prompt"])
def test_generation_end_to_end(Tp):
    """The prompt is longer than the window. 30 tokens go through the decode kernel, 70 through the causal flash
    forward (a prompt of >= 64 tokens into an empty cache)."""
    N = 24
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    prompt = torch.randint(0, V, (3, Tp), generator=torch.Generator().manual_seed(2))
    want, dists = _loop_greedy(gpu, prompt.to(DEV), N)
    fallback.reset()
    r = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert torch.equal(r.tokens.cpu(), want)
    assert gpu.rnnGetPreviousState("decoder_0")["kv"].shape == (3, Tp + N - 1, 2 * 128)   # the cache keeps every row
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
    # the fp8 cache: windowed generation runs on the kernels too
    gpu.rnnClearPreviousState()
    gpu.rnnSetCacheDataType("fp8")
    r8 = gpu.generate(prompt.to(DEV), maxNewTokens=N, lengthPenalty=0.0)
    assert r8.tokens.shape == r.tokens.shape and fallback.count() == 0, fallback.summary()


def test_ragged_prompts_equal_every_row_alone():
    net = _lm(DataType.BFLOAT16, DEV)
    N, lens = 16, [30, 23]
    prompt = torch.randint(0, V, (2, 30), generator=torch.Generator().manual_seed(4)).to(DEV)
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


def _decode_step_kernels(net):
    from torch.profiler import ProfilerActivity, profile
    x = torch.randint(0, V, (4, 40), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(37, 40)]
    net.rnnClearPreviousState()
    net.rnnTimeStep(x[:, :37].contiguous())
    net.rnnTimeStep(steps[0])
    net.rnnTimeStep(steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_decode_step_launches_no_torch_compute_kernels_and_no_more_kernels_than_without_a_window():
    names = _decode_step_kernels(_lm(DataType.BFLOAT16, DEV))
    plain = _decode_step_kernels(_lm(DataType.BFLOAT16, DEV, None))
    assert len(names) > 10, names
    assert sum("attn_decode_win_kernel" in n for n in names) == 1, names       # the windowed block
    assert sum("attn_decode_gqa_kernel" in n for n in names) == 1, names       # the block without a window
    assert sum("attn_decode_win_kernel" in n for n in plain) == 0 and \
        sum("attn_decode_gqa_kernel" in n for n in plain) == 2, plain
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
    assert len(names) <= len(plain), (len(names), len(plain))
