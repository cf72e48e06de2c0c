#!/usr/bin/env python3
"""Cached decoding measurements (csrc/attention_decode.hip, rnnTimeStep of the causal transformer layers).

  --kernel  GPU time of ``attn_decode`` for one new token (Tn = 1) over a history of L keys, L in {128, 1024, 4096},
            (B, H, D) in {(1, 12, 64), (32, 12, 64)}, bf16: once with splits = 1 and once with the default split
            count, in microseconds and as achieved read bandwidth of the cache (2 * L * E * 2 bytes per batch row).
            Every configuration is timed ``--passes`` times, alternating, so the log shows its own run-to-run spread.
            ``--sweep`` adds explicit split counts (for choosing the default).
  --model   tokens/s of ``TextGenerationTransformer(hidden=768, layers=12, heads=12)`` in bf16 at prefix lengths 128
            and 1024, for each minibatch size of ``--batch``: cached ``rnnTimeStep`` one token at a time against ``output()`` on the whole prefix per token
            (the only correct way without the cache). Host clock around work that ends in a device synchronise.

  --cache fp8  the fp8 key/value cache against the 16-bit one at the --kernel shapes, default splits, the variants
            alternating within every pass: the decode attention for one new token (bytes read: L * R per batch row
            against L * 4E) and the append of one new token; the fp8 output is compared bitwise with the 16-bit kernel
            on the dequantised cache. With --parent-lib also the 16-bit kernels of a kernel library built from the
            parent commit.

  --kv-heads N[,N..]  grouped-query attention: the decode attention and the append of one new token with 12 query
            heads of 64 over N key/value heads (12, the multi-head row, is always measured and is the baseline), at
            the --kernel shapes, 16-bit and fp8 cache, default splits, all variants alternating within every pass.
            Each row is reported against the 12-head row of the same run next to the ratio of the cache bytes read,
            which bounds the gain. With --parent-lib also the parent commit's multi-head decode, forward and
            backward kernels against this tree's (twice per pass: the spread of the parent alone is the yardstick).

  --rotary  rotary position embeddings (csrc/attention_rope.hip), 12 query heads of 64, bf16. (a) the fused
            ``attn_rope_append`` of one new token against the plain ``attn_kv_append`` at the same shape (with
            --parent-lib the parent commit's append: parent, ours, parent again in every pass, so the parent's own
            spread stands next to the ratio), Hkv in {12, 4}, batch 1 and 32, both cache formats. (b) ``attn_rope``
            alone at B = 32, T in {128, 512}: time and bytes per second (it reads and writes the Q and K columns once).

  --window W[,W..]  sliding-window decode (``attn_decode(..., window=W)``), 12 query heads of 64, Tn = 1, bf16, batch
            1 and 32, 12 and 4 key/value heads, 16-bit and fp8 cache, default splits: 4096 cached keys with each
            window against the kernel without a window at 4096 keys, and against the kernel without a window over a
            cache of W keys, which reads the same bytes and is the yardstick (ratio 1 = the window costs nothing
            beyond the keys it reads). All variants alternate within every pass.

Usage: python tools/bench_decode.py --kernel --model [--out profiles/decode_attention.txt]
       python tools/bench_decode.py --window 1024,256 [--out FILE]
       python tools/bench_decode.py --cache fp8 [--parent-lib PATH] [--out FILE]
       python tools/bench_decode.py --kv-heads 4,1 [--parent-lib PATH] [--out FILE]
       python tools/bench_decode.py --rotary [--parent-lib PATH] [--out FILE]"""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from deeplearning4j_amd.ops import transformer_native as TN  # noqa: E402
from deeplearning4j_amd.ops.timing import gpu_time  # noqa: E402

_out = None


def say(s=""):
    print(s, flush=True)
    if _out is not None:
        _out.write(s + "\n")
        _out.flush()


def kernel_mode(passes, sweep, reps):
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16
    say(f"== attn_decode, Tn = 1, bf16, GPU time per call (mean of {reps} back-to-back launches), {passes} passes")
    say("   bandwidth = 2*L*E*2 bytes per batch row / time; a cache that fits the last-level caches is re-read from them")
    for B, H, D in ((1, 12, 64), (32, 12, 64)):
        E = H * D
        for L in (128, 1024, 4096):
            pos = L - 1
            g = torch.Generator().manual_seed(L + B)
            qkv = (torch.randn(B, 1, 3 * E, generator=g) * 0.8).to(dt).to(dev)
            kv = (torch.randn(B, (L + 63) // 64 * 64, 2 * E, generator=g) * 0.8).to(dt).to(dev)
            assert TN.attn_kv_append(qkv, kv, H, pos) is kv
            default = TN.attn_decode_splits(B, 1, H, D, L)
            cands = [("splits=1", 1), (f"default={default}", default)]
            if sweep:
                cands += [(f"splits={s}", s) for s in (2, 4, 8, 16, 32, 64) if s <= (L + 63) // 64 and s != default]
            ref = TN.attn_decode(qkv, kv, H, pos, splits=1).float()
            times = {name: [] for name, _ in cands}
            for _ in range(passes):
                for name, s in cands:
                    times[name].append(gpu_time(lambda: TN.attn_decode(qkv, kv, H, pos, splits=s), reps=reps,
                                                warmup=3) * 1e3)
            nbytes = 2.0 * L * E * 2 * B
            for name, s in cands:
                t = sorted(times[name])
                med = t[len(t) // 2]
                diff = (TN.attn_decode(qkv, kv, H, pos, splits=s).float() - ref).abs().max().item()
                say(f"B={B:2d} H={H} D={D} L={L:4d} {name:12s}: " + " ".join(f"{v:7.2f}" for v in times[name]) +
                    f" us  median {med:7.2f} us  {nbytes / med / 1e3:7.1f} GB/s  (max diff vs splits=1 {diff:.1e})")
    say()


def _c_calls(lib):
    """(append, decode) straight on a kernel library's C ABI, argument types set by hand so that the parent commit's
    library can be driven too; ``fp8`` picks the fp8 entry points."""
    import ctypes
    vp, ci = ctypes.c_void_p, ctypes.c_int
    ptr = lambda t: None if t is None else vp(t.data_ptr())      # noqa: E731

    def append(fp8, qkv, kv, B, H, D, pos):
        f = lib.dl4j_attn_kv_append_fp8_dt if fp8 else lib.dl4j_attn_kv_append_dt
        f.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, ci, vp]
        return f(1, ptr(qkv), ptr(kv), B, 1, H, D, pos, kv.shape[1], vp(torch.cuda.current_stream().cuda_stream))

    def decode(fp8, qkv, kv, out, ws, B, H, D, pos, splits):
        f = lib.dl4j_attn_decode_fp8_dt if fp8 else lib.dl4j_attn_decode_dt
        f.argtypes = [ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.c_float, vp]
        return f(1, ptr(qkv), ptr(kv), ptr(out), ptr(ws), B, 1, H, D, pos, kv.shape[1], splits,
                 ctypes.c_float(D ** -0.5), vp(torch.cuda.current_stream().cuda_stream))
    return append, decode


def cache_fp8_mode(passes, reps, parent_lib):
    import ctypes
    from deeplearning4j_amd.ops import native
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    ours = _c_calls(ctypes.CDLL(native.KERNEL_LIB))
    parent = _c_calls(ctypes.CDLL(parent_lib)) if parent_lib else None
    say(f"== fp8 key/value cache against the 16-bit cache, Tn = 1, bf16, default splits, GPU time per call in us (mean "
        f"of {reps} back-to-back launches; median of {passes} passes, min .. max; the variants alternate within a pass)")
    say("   16-bit / fp8 = this tree's kernels" + ("; parent = the 16-bit kernels of the parent commit's library"
                                                  if parent else ""))
    say("   decode bandwidth = bytes of the valid cache rows (L * 4E, fp8 L * R per batch row) / time; a cache that "
        "fits the last-level caches is re-read from them")
    H, D = 12, 64
    E, R = H * D, TN.kv_fp8_row_bytes(12, 64)
    say(f"   H = {H}, D = {D}: R = {R} bytes per cached token against 4E = {4 * E}, ratio {R / (4 * E):.3f}")
    for B in (1, 32):
        for L in (128, 1024, 4096):
            pos = L - 1
            g = torch.Generator().manual_seed(L + B)
            qkv = (torch.randn(B, 1, 3 * E, generator=g) * 0.8).to(dt).to(dev)
            hist = (torch.randn(B, L, 3 * E, generator=g) * 0.8).to(dt).to(dev)
            tcap = (L + 63) // 64 * 64
            kv8 = torch.zeros(B, tcap, R, dtype=torch.uint8, device=dev)
            assert TN.attn_kv_append(hist, kv8, H, 0) is kv8 and TN.attn_kv_append(qkv, kv8, H, pos) is kv8
            kv16 = torch.zeros(B, tcap, 2 * E, dtype=dt, device=dev)
            kv16[:, :L] = TN.kv_fp8_dequantize_reference(kv8[:, :L], H, D, dt)
            splits = TN.attn_decode_splits(B, 1, H, D, L)
            ws = torch.empty(max(1, B * H * splits * (D + 2)), dtype=torch.float32, device=dev)
            variants = [("16-bit", ours, False, kv16), ("fp8", ours, True, kv8)]
            if parent:
                variants.insert(0, ("parent", parent, False, kv16))
            outs = [torch.empty(B, 1, E, dtype=dt, device=dev) for _ in variants]
            for (_, (_, dec), f8, kv), o in zip(variants, outs):
                assert dec(f8, qkv, kv, o, ws, B, H, D, pos, splits) == 0
            torch.cuda.synchronize()
            same = all(torch.equal(outs[0], o) for o in outs[1:])
            td, ta = [[] for _ in variants], [[] for _ in variants]
            for _ in range(passes):
                for i, (_, (app, dec), f8, kv) in enumerate(variants):
                    td[i].append(gpu_time(lambda: dec(f8, qkv, kv, outs[i], ws, B, H, D, pos, splits), reps=reps,
                                          warmup=3) * 1e3)
                for i, (_, (app, dec), f8, kv) in enumerate(variants):
                    ta[i].append(gpu_time(lambda: app(f8, qkv, kv, B, H, D, pos), reps=reps, warmup=3) * 1e3)
            for what, times in (("decode", td), ("append", ta)):
                line = f"{what} B={B:2d} L={L:4d} splits={splits:2d}:"
                med = []
                for (name, _, f8, _), t in zip(variants, times):
                    t = sorted(t)
                    med.append(t[len(t) // 2])
                    line += f"  {name} {med[-1]:7.2f} ({t[0]:.2f} .. {t[-1]:.2f})"
                    if what == "decode":
                        line += f" {B * L * (R if f8 else 4 * E) / med[-1] / 1e3:7.1f} GB/s"
                line += f"  16-bit / fp8 time {med[-2] / med[-1]:5.2f}x"
                if parent:
                    line += f"  16-bit / parent time {med[1] / med[0]:5.3f}x"
                if what == "decode":
                    line += f"  outputs bitwise equal: {same}"
                say(line)
    say()


def _stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def gqa_mode(kv_heads, passes, reps, parent_lib):
    """12 query heads of 64 over Hkv key/value heads, Tn = 1: decode and append, 16-bit and fp8 cache."""
    import ctypes
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    H, D = 12, 64
    E = H * D
    heads = [H] + [h for h in kv_heads if h != H]
    parent = _c_calls(ctypes.CDLL(parent_lib)) if parent_lib else None
    say(f"== grouped-query decode, H = {H} query heads of {D}, Tn = 1, bf16, default splits, GPU time per call in us "
        f"(mean of {reps} back-to-back launches; median of {passes} passes, min .. max; all variants alternate within "
        "a pass)")
    say("   x = time of the Hkv = 12 row of the same cache format / this row's time; bytes = this row's cache bytes "
        "read / the 12-head row's (the bound on 1/x); GB/s = valid cache bytes / time")
    for B in (1, 32):
        for L in (128, 1024, 4096):
            pos, tcap = L - 1, (L + 63) // 64 * 64
            variants = []                                        # (name, Hkv, fp8, run decode, run append, bytes)
            for fp8 in (False, True):
                for Hkv in heads:
                    Ekv = Hkv * D
                    g = torch.Generator().manual_seed(L + B + Hkv)
                    qkv = (torch.randn(B, 1, E + 2 * Ekv, generator=g) * 0.8).to(dt).to(dev)
                    hist = (torch.randn(B, L, E + 2 * Ekv, generator=g) * 0.8).to(dt).to(dev)
                    R = TN.kv_fp8_row_bytes(Hkv, D) if fp8 else 4 * Ekv
                    kv = torch.zeros(B, tcap, R if fp8 else 2 * Ekv, dtype=torch.uint8 if fp8 else dt, device=dev)
                    assert TN.attn_kv_append(hist, kv, H, 0, Hkv=Hkv) is kv
                    assert TN.attn_kv_append(qkv, kv, H, pos, Hkv=Hkv) is kv
                    splits = TN.attn_decode_splits(B, 1, H, D, L, Hkv=Hkv)
                    assert TN.attn_decode(qkv, kv, H, pos, splits=splits, Hkv=Hkv) is not None
                    variants.append((f"{'fp8' if fp8 else '16-bit'} Hkv={Hkv:2d} S={splits:2d}", Hkv, fp8,
                                     lambda q=qkv, c=kv, k=Hkv, s=splits: TN.attn_decode(q, c, H, pos, splits=s, Hkv=k),
                                     lambda q=qkv, c=kv, k=Hkv: TN.attn_kv_append(q, c, H, pos, Hkv=k), B * L * R))
            td, ta = [[] for _ in variants], [[] for _ in variants]
            for _ in range(passes):
                for i, v in enumerate(variants):
                    td[i].append(gpu_time(v[3], reps=reps, warmup=3) * 1e3)
                for i, v in enumerate(variants):
                    ta[i].append(gpu_time(v[4], reps=reps, warmup=3) * 1e3)
            base = {}
            for i, (name, Hkv, fp8, _, _, nbytes) in enumerate(variants):
                md, lo, hi = _stats(td[i])
                ma, _, _ = _stats(ta[i])
                if Hkv == H:
                    base[fp8] = (md, nbytes)
                bd, bb = base[fp8]
                say(f"B={B:2d} L={L:4d} {name}: decode {md:7.2f} ({lo:.2f} .. {hi:.2f}) us  x {bd / md:5.2f}  bytes "
                    f"{nbytes / bb:5.3f}  {nbytes / md / 1e3:7.1f} GB/s | append {ma:6.2f} us")
    say()
    if parent is None:
        return
    from deeplearning4j_amd.ops import native
    ours = _c_calls(ctypes.CDLL(native.KERNEL_LIB))
    say("== the multi-head kernels of this tree against the parent commit's library, alternating on one device: "
        "parent, ours, parent again in every pass; 'parent spread' = (max - min) / median over ALL parent timings, "
        "ours / parent = ratio of the medians (above 1 = slower)")
    vp, ci = ctypes.c_void_p, ctypes.c_int

    def flash(lib, B, T):
        """(forward, backward) closures on a library's multi-head entry points."""
        g = torch.Generator().manual_seed(T)
        qkv = (torch.randn(B, T, 3 * E, generator=g) * 0.8).to(dt).to(dev)
        dout = torch.randn(B, T, E, generator=g).to(dt).to(dev)
        out, dq = torch.empty(B, T, E, dtype=dt, device=dev), torch.empty_like(qkv)
        lse, dd = torch.empty(B, H, T, device=dev), torch.empty(B, H, T, device=dev)
        st = lambda: vp(torch.cuda.current_stream().cuda_stream)                 # noqa: E731
        fw, bw = lib.dl4j_attn_fwd_dt, lib.dl4j_attn_bwd_dt
        fw.argtypes = [ci, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, ci, vp]
        bw.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, ci, vp]
        sc = ctypes.c_float(D ** -0.5)
        f = lambda: fw(1, qkv.data_ptr(), None, out.data_ptr(), lse.data_ptr(), B, T, H, D, sc, 1, st())  # noqa: E731
        b = lambda: bw(1, qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), None, lse.data_ptr(),  # noqa: E731
                       dd.data_ptr(), dq.data_ptr(), B, T, H, D, sc, 1, st())
        assert f() == 0 and b() == 0
        return f, b, dq

    def ab(label, run_parent, run_ours):
        tp, to = [], []
        for _ in range(passes):
            tp.append(gpu_time(run_parent, reps=reps, warmup=3) * 1e3)
            to.append(gpu_time(run_ours, reps=reps, warmup=3) * 1e3)
            tp.append(gpu_time(run_parent, reps=reps, warmup=3) * 1e3)
        mp, lp, hp = _stats(tp)
        mo, lo, ho = _stats(to)
        say(f"{label}: parent {mp:8.2f} ({lp:.2f} .. {hp:.2f}) us, spread {(hp - lp) / mp * 100:4.1f} %  "
            f"ours {mo:8.2f} ({lo:.2f} .. {ho:.2f}) us  ours / parent {mo / mp:6.3f}x")

    for B, T in ((8, 512), (32, 128)):
        fp, bp, dqp = flash(ctypes.CDLL(parent_lib), B, T)
        fo, bo, dqo = flash(ctypes.CDLL(native.KERNEL_LIB), B, T)
        torch.cuda.synchronize()
        say(f"flash B={B} T={T} causal: backward outputs bitwise equal: {torch.equal(dqp, dqo)}")
        ab(f"forward  B={B:2d} T={T:3d}", fp, fo)
        ab(f"backward B={B:2d} T={T:3d}", bp, bo)
    for B in (1, 32):
        for L in (128, 1024, 4096):
            pos, tcap = L - 1, (L + 63) // 64 * 64
            g = torch.Generator().manual_seed(L + B)
            qkv = (torch.randn(B, 1, 3 * E, generator=g) * 0.8).to(dt).to(dev)
            kv = (torch.randn(B, tcap, 2 * E, generator=g) * 0.8).to(dt).to(dev)
            splits = TN.attn_decode_splits(B, 1, H, D, L)
            ws = torch.empty(max(1, B * H * splits * (D + 2)), dtype=torch.float32, device=dev)
            o1, o2 = torch.empty(B, 1, E, dtype=dt, device=dev), torch.empty(B, 1, E, dtype=dt, device=dev)
            assert parent[1](False, qkv, kv, o1, ws, B, H, D, pos, splits) == 0
            assert ours[1](False, qkv, kv, o2, ws, B, H, D, pos, splits) == 0
            torch.cuda.synchronize()
            same = torch.equal(o1, o2)
            ab(f"decode   B={B:2d} L={L:4d} splits={splits:2d} (bitwise equal: {same})",
               lambda: parent[1](False, qkv, kv, o1, ws, B, H, D, pos, splits),
               lambda: ours[1](False, qkv, kv, o2, ws, B, H, D, pos, splits))
    say()


def window_mode(windows, passes, reps):
    """Tn = 1 over 4096 cached keys with a window against no window, and against no window over W keys."""
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    H, D, L = 12, 64, 4096
    E = H * D
    say(f"== sliding-window decode, H = {H} query heads of {D}, Tn = 1, bf16, default splits S, GPU time per call in us "
        f"(mean of {reps} back-to-back launches; median of {passes} passes, min .. max; all variants alternate within "
        "a pass)")
    say(f"   full = no window over {L} keys; W = window W over {L} keys; short = no window over a cache of W keys (the "
        "same bytes read: the yardstick); W / short = ratio of the medians, full / W = the gain")
    for B in (1, 32):
        for Hkv in (12, 4):
            for fp8 in (False, True):
                Ekv = Hkv * D
                R = TN.kv_fp8_row_bytes(Hkv, D) if fp8 else 2 * Ekv

                def cache(n):
                    g = torch.Generator().manual_seed(n + B + Hkv)
                    qkv = (torch.randn(B, 1, E + 2 * Ekv, generator=g) * 0.8).to(dt).to(dev)
                    hist = (torch.randn(B, n, E + 2 * Ekv, generator=g) * 0.8).to(dt).to(dev)
                    kv = torch.zeros(B, (n + 63) // 64 * 64, R, dtype=torch.uint8 if fp8 else dt, device=dev)
                    assert TN.attn_kv_append(hist, kv, H, 0, Hkv=Hkv) is kv
                    return qkv, kv

                qkv, kv = cache(L)
                variants = [("full", TN.attn_decode_splits(B, 1, H, D, L, Hkv=Hkv),
                             lambda q=qkv, c=kv: TN.attn_decode(q, c, H, L - 1, Hkv=Hkv))]
                for W in windows:
                    qs, ks = cache(W)
                    variants.append((f"W={W}", TN.attn_decode_splits(B, 1, H, D, L, Hkv=Hkv, window=W),
                                     lambda q=qkv, c=kv, w=W: TN.attn_decode(q, c, H, L - 1, Hkv=Hkv, window=w)))
                    variants.append((f"short={W}", TN.attn_decode_splits(B, 1, H, D, W, Hkv=Hkv),
                                     lambda q=qs, c=ks, w=W: TN.attn_decode(q, c, H, w - 1, Hkv=Hkv)))
                for v in variants:
                    assert v[2]() is not None
                t = [[] for _ in variants]
                for _ in range(passes):
                    for i, v in enumerate(variants):
                        t[i].append(gpu_time(v[2], reps=reps, warmup=3) * 1e3)
                med = {}
                head = f"B={B:2d} Hkv={Hkv:2d} {'fp8   ' if fp8 else '16-bit'}"
                for (name, S, _), ti in zip(variants, t):
                    m, lo, hi = _stats(ti)
                    med[name] = m
                    line = f"{head} {name:10s} S={S:2d}: {m:7.2f} ({lo:.2f} .. {hi:.2f}) us, spread {(hi - lo) / m * 100:4.1f} %"
                    if name.startswith("short="):
                        w = name[6:]
                        line += f"  W / short {med['W=' + w] / m:5.3f}  full / W {med['full'] / med['W=' + w]:5.2f}x"
                    say(line)
    say()


def rotary_mode(passes, reps, parent_lib):
    import ctypes
    from deeplearning4j_amd.ops import native
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    H, D, theta = 12, 64, 10000.0
    E = H * D
    lib = ctypes.CDLL(parent_lib if parent_lib else native.KERNEL_LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    who = "the parent commit's library" if parent_lib else "this tree (its append kernels are the parent's, unchanged)"
    say(f"== attn_rope_append against attn_kv_append of {who}: H = {H} query heads of {D}, Tn = 1, bf16, pos = 1023 of "
        f"1024 rows, GPU time per call in us (mean of {reps} back-to-back launches; median of {passes} passes, min .. "
        "max); every pass runs plain, fused, plain: 'spread' = (max - min) / median over ALL plain timings, fused / "
        "plain = ratio of the medians (above 1 = slower)")
    for fp8 in (False, True):
        for Hkv in (12, 4):
            for B in (1, 32):
                Ekv, pos, tcap = Hkv * D, 1023, 1024
                g = torch.Generator().manual_seed(B + Hkv)
                qkv = (torch.randn(B, 1, E + 2 * Ekv, generator=g) * 0.8).to(dt).to(dev)
                width = TN.kv_fp8_row_bytes(Hkv, D) if fp8 else 2 * Ekv
                kv = torch.zeros(B, tcap, width, dtype=torch.uint8 if fp8 else dt, device=dev)
                f = lib.dl4j_attn_kv_append_fp8_gqa_dt if fp8 else lib.dl4j_attn_kv_append_gqa_dt
                f.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
                st = lambda: vp(torch.cuda.current_stream().cuda_stream)                 # noqa: E731
                plain = lambda: f(1, qkv.data_ptr(), kv.data_ptr(), B, 1, H, Hkv, D, pos, tcap, st())   # noqa: E731
                fused = lambda: TN.attn_rope_append(qkv, kv, H, pos, theta, Hkv=Hkv)     # noqa: E731
                assert plain() == 0 and fused() is kv
                tp, tf = [], []
                for _ in range(passes):
                    tp.append(gpu_time(plain, reps=reps, warmup=3) * 1e3)
                    tf.append(gpu_time(fused, reps=reps, warmup=3) * 1e3)
                    tp.append(gpu_time(plain, reps=reps, warmup=3) * 1e3)
                mp, lp, hp = _stats(tp)
                mf, lf, hf = _stats(tf)
                say(f"{'fp8   ' if fp8 else '16-bit'} Hkv={Hkv:2d} B={B:2d}: plain {mp:6.2f} ({lp:.2f} .. {hp:.2f}) us, "
                    f"spread {(hp - lp) / mp * 100:4.1f} %  fused {mf:6.2f} ({lf:.2f} .. {hf:.2f}) us  fused / plain "
                    f"{mf / mp:5.3f}x")
    say()
    say(f"== attn_rope alone (training and prompts): B = 32, H = {H}, D = {D}, bf16, in place; bytes = the Q and K "
        "columns read once and written once")
    for Hkv in (12, 4):
        for T in (128, 512):
            g = torch.Generator().manual_seed(T + Hkv)
            qkv = (torch.randn(32, T, E + 2 * Hkv * D, generator=g) * 0.8).to(dt).to(dev)
            assert TN.attn_rope(qkv, H, 0, theta, Hkv=Hkv) is qkv
            t = [gpu_time(lambda: TN.attn_rope(qkv, H, 0, theta, Hkv=Hkv), reps=reps, warmup=3) * 1e3
                 for _ in range(passes)]
            m, lo, hi = _stats(t)
            nbytes = 2.0 * 32 * T * (H + Hkv) * D * 2
            say(f"Hkv={Hkv:2d} T={T:3d}: {m:7.2f} ({lo:.2f} .. {hi:.2f}) us  {nbytes / 1e6:6.1f} MB  "
                f"{nbytes / m / 1e3:7.1f} GB/s")
    say()


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def model_mode(batches, n_cached, n_full):
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    dev = torch.device("cuda", 0)
    V = 77
    net = TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=768, layers=12, heads=12, maxPositions=2048,
                                    dataType=DataType.BFLOAT16).init(device=dev)
    for batch in batches:
        _model_rows(net, V, dev, batch, n_cached, n_full)


def _model_rows(net, V, dev, batch, n_cached, n_full):
    say(f"== TextGenerationTransformer(hidden=768, layers=12, heads=12) bf16, batch {batch}: generated tokens/s")
    for P in (128, 1024):
        x = torch.randint(0, V, (batch, P + max(n_cached, n_full) + 4), generator=torch.Generator().manual_seed(P)).to(dev)

        def cached(n, warm):
            net.rnnClearPreviousState()
            net.rnnTimeStep(x[:, :P - warm])                                   # the prompt
            for t in range(P - warm, P):
                net.rnnTimeStep(x[:, t:t + 1])                                 # warm the single-token shapes
            last = [None]

            def run():
                for t in range(P, P + n):
                    last[0] = net.rnnTimeStep(x[:, t:t + 1])[0]
            return _sync_time(run), last[0]

        def full(n):
            last = [None]

            def run():
                for t in range(P, P + n):
                    last[0] = net.output(x[:, :t + 1])[0][:, :, -1:]
            return _sync_time(run), last[0]

        cached(2, 2)
        full(n_full)                                                           # warm-up of both paths: every prefix
                                                                               # length is a GEMM shape of its own
        tc, yc = cached(n_cached, 2)
        tf, yf = full(n_full)
        _, yc_at = cached(n_full, 2)                                           # same last position as the full run
        agree = (yc_at - yf).abs().max().item()
        rc, rf = batch * n_cached / tc, batch * n_full / tf
        say(f"prefix {P:4d}: cached rnnTimeStep {rc:9.1f} tok/s ({tc / n_cached * 1e3:7.2f} ms/step, {n_cached} steps)"
            f" | output() on the prefix {rf:9.1f} tok/s ({tf / n_full * 1e3:7.2f} ms/step, {n_full} steps)"
            f" | factor {rc / rf:6.2f}x | max |p_cached - p_full| {agree:.2e}")
    say()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="--kernel: also time explicit split counts")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", default="1,32", help="--model: minibatch sizes, comma separated")
    ap.add_argument("--cached-steps", type=int, default=64)
    ap.add_argument("--full-steps", type=int, default=16)
    ap.add_argument("--cache", choices=["fp8"], default=None,
                    help="compare the fp8 key/value cache's kernels with the 16-bit ones")
    ap.add_argument("--kv-heads", default=None,
                    help="grouped-query attention: key/value head counts (divisors of 12, comma separated) to compare "
                         "with the 12-head row")
    ap.add_argument("--rotary", action="store_true",
                    help="rotary embeddings: the fused rotate-and-append against the plain append, and attn_rope alone")
    ap.add_argument("--window", default=None,
                    help="comma-separated windows: the windowed decode at 4096 keys against no window and against "
                         "no window over W keys")
    ap.add_argument("--parent-lib", default=None,
                    help="--cache / --kv-heads / --rotary: kernel library built from the parent commit")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not (a.kernel or a.model or a.cache or a.kv_heads or a.rotary or a.window):
        ap.error("give --kernel, --model, --cache fp8, --kv-heads N, --rotary and / or --window W")
    windows = [int(w) for w in a.window.split(",")] if a.window else []
    if any(w < 1 for w in windows):
        ap.error("--window: every window must be a positive integer")
    kv_heads = [int(h) for h in a.kv_heads.split(",")] if a.kv_heads else []
    if any(h < 1 or 12 % h for h in kv_heads):
        ap.error("--kv-heads: every count must divide the 12 query heads")
    if not torch.cuda.is_available():
        sys.exit("bench_decode.py measures on the GPU; no device found")
    global _out
    if a.out:
        _out = open(a.out, "w")
    say(f"# tools/bench_decode.py {' '.join(sys.argv[1:])}   ({torch.cuda.get_device_name(0)})")
    if a.kernel:
        kernel_mode(a.passes, a.sweep, a.reps)
    if a.model:
        model_mode([int(b) for b in a.batch.split(",")], a.cached_steps, a.full_steps)
    if a.cache:
        cache_fp8_mode(max(a.passes, 5), a.reps, a.parent_lib)
    if kv_heads:
        gqa_mode(kv_heads, max(a.passes, 5), a.reps, a.parent_lib)
    if a.rotary:
        rotary_mode(max(a.passes, 5), a.reps, a.parent_lib)
    if windows:
        window_mode(windows, max(a.passes, 5), a.reps)
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()
