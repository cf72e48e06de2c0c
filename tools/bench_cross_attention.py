#!/usr/bin/env python3
"""Cross-attention measurements (csrc/attention_cross.hip, TransformerDecoderLayer, TransformerSeq2Seq).

  --kernel  GPU time of the cross kernels, forward and forward + backward, bf16, (B, H, D) = (32, 12, 64):
            * at Tq = Tk in {128, 512} next to the self-attention kernels of csrc/attention.hip on the same shape (the
              same arithmetic; the yardstick);
            * at (Tq, Tk) in {(128, 512), (1, 512)} next to ``cross_attention_fwd_explicit`` /
              ``cross_attention_bwd_explicit`` on the GPU, which materialise P[B, H, Tq, Tk] in fp32 and were the only
              way to compute this shape before the kernels.
            Every configuration is timed ``--passes`` times, alternating, so the log shows its own run-to-run spread.
  --model   tokens/s of a ``TransformerSeq2Seq`` training step (hidden 768, 6 + 6 layers, 12 heads, source 128 /
            target 128, batch 32, bf16; target tokens per second) and of generation at batch 1 and 32: the source
            once, then ``rnnTimeStep(None, token)`` per token. Host clock around work that ends in a device
            synchronise.

Usage: python tools/bench_cross_attention.py --kernel --model [--out profiles/cross_attention.txt]"""
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


def _row(label, ts):
    t = sorted(ts)
    say(f"  {label:34s}: " + " ".join(f"{v:8.1f}" for v in ts) + f" us  median {t[len(t) // 2]:8.1f} us")
    return t[len(t) // 2]


def kernel_mode(passes, reps):
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16
    B, H, D = 32, 12, 64
    E = H * D
    say(f"== cross attention kernels, bf16, (B, H, D) = ({B}, {H}, {D}); GPU time per call in microseconds (mean of "
        f"{reps} back-to-back launches), {passes} alternating passes")

    def operands(Tq, Tk):
        g = torch.Generator().manual_seed(Tq * 7 + Tk)
        q = (torch.randn(B, Tq, E, generator=g) * 0.8).to(dt).to(dev)
        kv = (torch.randn(B, Tk, 2 * E, generator=g) * 0.8).to(dt).to(dev)
        dout = torch.randn(B, Tq, E, generator=g).to(dt).to(dev)
        return q, kv, dout

    for T in (128, 512):
        q, kv, dout = operands(T, T)
        qkv = torch.cat([q, kv], 2).contiguous()
        out, lse = TN.cross_attn_fwd(q, kv, H)
        so, sl = TN.attn_fwd(qkv, H)
        agree = (out.float() - so.float()).abs().max().item()
        cands = {
            "cross fwd": lambda: TN.cross_attn_fwd(q, kv, H),
            "self  fwd": lambda: TN.attn_fwd(qkv, H),
            "cross fwd+bwd": lambda: TN.cross_attn_bwd(q, kv, *TN.cross_attn_fwd(q, kv, H), dout, H),
            "self  fwd+bwd": lambda: TN.attn_bwd(qkv, *TN.attn_fwd(qkv, H), dout, H),
        }
        times = {k: [] for k in cands}
        for _ in range(passes):
            for k, fn in cands.items():
                times[k].append(gpu_time(fn, reps=reps, warmup=3) * 1e3)
        say(f"Tq = Tk = {T} (max |cross - self| of the outputs {agree:.1e})")
        med = {k: _row(k, v) for k, v in times.items()}
        say(f"  cross / self: fwd {med['cross fwd'] / med['self  fwd']:.3f}, "
            f"fwd+bwd {med['cross fwd+bwd'] / med['self  fwd+bwd']:.3f}")
    for Tq, Tk in ((128, 512), (1, 512)):
        q, kv, dout = operands(Tq, Tk)

        def explicit_fb():
            o, ctx = TN.cross_attention_fwd_explicit(q, kv, H)
            return TN.cross_attention_bwd_explicit(ctx, dout, dt)

        cands = {
            "cross fwd": lambda: TN.cross_attn_fwd(q, kv, H),
            "explicit torch fwd": lambda: TN.cross_attention_fwd_explicit(q, kv, H),
            "cross fwd+bwd": lambda: TN.cross_attn_bwd(q, kv, *TN.cross_attn_fwd(q, kv, H), dout, H),
            "explicit torch fwd+bwd": explicit_fb,
        }
        times = {k: [] for k in cands}
        for _ in range(passes):
            for k, fn in cands.items():
                times[k].append(gpu_time(fn, reps=max(5, reps // 5), warmup=2) * 1e3)
        say(f"Tq = {Tq}, Tk = {Tk}")
        med = {k: _row(k, v) for k, v in times.items()}
        say(f"  explicit / cross: fwd {med['explicit torch fwd'] / med['cross fwd']:.1f}x, "
            f"fwd+bwd {med['explicit torch fwd+bwd'] / med['cross fwd+bwd']:.1f}x")
    say()


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def model_mode(passes, train_steps, gen_steps):
    from deeplearning4j_amd.models import TransformerSeq2Seq
    from deeplearning4j_amd.nn.conf import DataType
    dev = torch.device("cuda", 0)
    V, Ts, Tt, MB = 1000, 128, 128, 32
    net = TransformerSeq2Seq(numLabels=V, inputShape=[Ts, Tt], hidden=768, layers=6, heads=12, maxPositions=512,
                             dataType=DataType.BFLOAT16).init(device=dev)
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, V, (MB, Ts), generator=g).to(dev)
    tgt = torch.randint(0, V, (MB, Tt), generator=g).to(dev)
    lab = torch.nn.functional.one_hot(torch.roll(tgt, -1, 1), V).permute(0, 2, 1).float().contiguous()
    say(f"== TransformerSeq2Seq(hidden=768, layers=6+6, heads=12) bf16, source {Ts} / target {Tt}")

    def train():
        for _ in range(train_steps):
            net.fit([src, tgt], [lab])
    net.fit([src, tgt], [lab])
    net.fit([src, tgt], [lab])
    ts = [_sync_time(train) for _ in range(passes)]
    say(f"training step, batch {MB}: " + " ".join(f"{t / train_steps * 1e3:7.2f}" for t in ts) + " ms/step  "
        + " ".join(f"{MB * Tt * train_steps / t:9.0f}" for t in ts) + " target tok/s")
    for mb in (1, 32):
        s, t = src[:mb].contiguous(), tgt[:mb].contiguous()

        def gen():
            net.rnnClearPreviousState()
            net.rnnTimeStep(s, t[:, :1])
            for i in range(1, gen_steps):
                net.rnnTimeStep(None, t[:, i:i + 1])
        gen()
        ts = [_sync_time(gen) for _ in range(passes)]
        say(f"generation, batch {mb:2d}, {gen_steps} tokens after the source: " +
            " ".join(f"{x / gen_steps * 1e3:6.2f}" for x in ts) + " ms/token  " +
            " ".join(f"{mb * gen_steps / x:8.0f}" for x in ts) + " tok/s")
    from deeplearning4j_amd.ops import fallback
    say(f"fallbacks recorded: {fallback.count('attention')} attention")
    say()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--gen-steps", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not (a.kernel or a.model):
        ap.error("give --kernel and / or --model")
    if not torch.cuda.is_available():
        sys.exit("bench_cross_attention.py measures on the GPU; no device found")
    global _out
    if a.out:
        _out = open(a.out, "w")
    say(f"# tools/bench_cross_attention.py {' '.join(sys.argv[1:])}   ({torch.cuda.get_device_name(0)})")
    if a.kernel:
        kernel_mode(a.passes, a.reps)
    if a.model:
        model_mode(a.passes, a.train_steps, a.gen_steps)
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()
