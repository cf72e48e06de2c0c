#!/usr/bin/env python3
"""Sliding-window flash attention timings (the WIN instances of csrc/attention_body.h): the causal forward and the
forward + backward of ``attn_fwd`` / ``attn_bwd`` with a window against the same calls without one, batch 32, 12 heads
of 64, bf16, T in {2048, 4096}, W in {256, 1024}. Next to every time stands the share of (query block, key block)
pairs the windowed kernels visit of those the causal kernels visit, which is what the time should follow.
All variants of a shape alternate within every pass; the log shows the spread between passes.

Usage: python tools/bench_window_attention.py [--windows 256,1024] [--lengths 2048,4096] [--out FILE]"""
import argparse
import sys

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


def visited(T, W=None, blk=64):
    """(query block, key block) pairs the forward / dQ kernels visit: key blocks [first, last] of every query tile."""
    n = 0
    for q0 in range(0, T, blk):
        first = 0 if W is None else max(0, q0 - W + 1) // blk
        n += q0 // blk - first + 1
    return n


def _stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", default="256,1024")
    ap.add_argument("--lengths", default="2048,4096")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=12)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_window_attention.py measures on the GPU; no device found")
    if a.out:
        _out = open(a.out, "w")
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    B, H, Hkv, D = a.batch, 12, a.kv_heads, 64
    windows = [int(w) for w in a.windows.split(",")]
    say(f"# tools/bench_window_attention.py {' '.join(sys.argv[1:])}   ({torch.cuda.get_device_name(0)})")
    say(f"== causal flash attention with a window against none, B = {B}, H = {H} heads of {D} over {Hkv} key/value heads, "
        f"bf16: GPU time per call in ms (mean of {a.reps} back-to-back launches; median of {a.passes} passes, min .. "
        "max; the variants alternate within a pass); blocks = key blocks visited / the causal kernel's; time = this "
        "row's / the causal row's")
    for T in (int(t) for t in a.lengths.split(",")):
        g = torch.Generator().manual_seed(T)
        qkv = (torch.randn(B, T, (H + 2 * Hkv) * D, generator=g) * 0.8).to(dt).to(dev)
        dout = torch.randn(B, T, H * D, generator=g).to(dt).to(dev)
        dqkv = torch.empty_like(qkv)
        variants = []
        for W in [None] + windows:
            out, lse = TN.attn_fwd(qkv, H, None, True, Hkv=Hkv, window=W)
            fwd = lambda w=W: TN.attn_fwd(qkv, H, None, True, Hkv=Hkv, window=w)                       # noqa: E731
            bwd = lambda w=W, o=out, l=lse: TN.attn_bwd(qkv, o, l, dout, H, None, True, Hkv=Hkv, dqkv=dqkv,  # noqa: E731
                                                        window=w)
            assert bwd() is not None
            variants.append((W, fwd, bwd))
        tf, tb = [[] for _ in variants], [[] for _ in variants]
        for _ in range(a.passes):
            for i, (_, fwd, bwd) in enumerate(variants):
                tf[i].append(gpu_time(fwd, reps=a.reps, warmup=2))
            for i, (_, fwd, bwd) in enumerate(variants):
                tb[i].append(gpu_time(bwd, reps=a.reps, warmup=2))
        base = None
        for (W, _, _), f, b in zip(variants, tf, tb):
            mf, lf, hf = _stats(f)
            mb, lb, hb = _stats(b)
            if base is None:
                base = (mf, mb)
            share = visited(T, W) / visited(T)
            say(f"T={T:4d} W={'none' if W is None else W:>4}: blocks {share:5.3f} | forward {mf:7.3f} ({lf:.3f} .. {hf:.3f})"
                f" time {mf / base[0]:5.3f} | backward {mb:7.3f} ({lb:.3f} .. {hb:.3f}) time {mb / base[1]:5.3f} | "
                f"forward + backward {mf + mb:7.3f} time {(mf + mb) / (base[0] + base[1]):5.3f}")
    say()
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()
