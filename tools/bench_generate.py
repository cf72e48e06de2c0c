#!/usr/bin/env python3
"""Token generation measurements (csrc/generation.hip, rnnReorderState, generate()).

  --sampler  GPU time of the row sampler at R in {1, 32, 256} rows and V in {77, 32000, 128000}, bf16 probabilities,
             for greedy, plain sampling and temperature 0.8 / top-k 50 / top-p 0.9, against the torch ops a user
             would write on the same tensor (fp32 copy, topk / sort, cumsum, multinomial).
  --gather   GPU time of the cache gather per layer at the 12-layer model's shapes (C = 2 * 768, capacity 256, 128
             or 192 valid rows, 4 / 128 rows = batch 1 / 32 with 4 beams) against index_select of the valid rows.
  --model    tokens/s of generate() on TextGenerationTransformer(hidden=768, layers=12, heads=12) in bf16, prefix
             128, batch 1 / 32: greedy, sampling and numBeams=4, against the loop written on the public API before
             generate() existed (rnnTimeStep, torch.multinomial on the device, one .item() eos test per step; that
             loop touches nothing this tool's tree changed). Host clock around work that ends in a device synchronise.

Usage: python tools/bench_generate.py --sampler --gather --model [--out profiles/generation.txt]"""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from deeplearning4j_amd.ops import generation_native as GN  # noqa: E402
from deeplearning4j_amd.ops.nn_misc import PhiloxStream  # noqa: E402
from deeplearning4j_amd.ops.timing import gpu_time  # noqa: E402

_out = None
DEV = torch.device("cuda", 0)


def say(s=""):
    print(s, flush=True)
    if _out is not None:
        _out.write(s + "\n")
        _out.flush()


def _med(fn, passes, reps):
    t = sorted(gpu_time(fn, reps=reps, warmup=3) * 1e3 for _ in range(passes))
    return t[len(t) // 2], t[0], t[-1]


def _torch_sample(p, temperature, topK, topP):
    x = p.float()
    if topK:
        x, idx = torch.topk(x, topK, dim=1)
    else:
        x, idx = torch.sort(x, dim=1, descending=True)
    if temperature != 1.0:
        x = x ** (1.0 / temperature)
    if topP < 1.0:
        c = torch.cumsum(x, 1)
        x = x * ((c - x) < topP * c[:, -1:])
    return idx.gather(1, torch.multinomial(x, 1))


def sampler_mode(passes, reps):
    say(f"== row sampler, bf16 probabilities, GPU time per call in us (median of {passes} passes of {reps} launches; "
        "min .. max)")
    say("   torch = fp32 copy + topk (top-k on) or sort + cumsum (top-p on) + multinomial on the same tensor; greedy = "
        "argmax")
    rng = PhiloxStream(DEV)
    for R in (1, 32, 256):
        for V in (77, 32000, 128000):
            g = torch.Generator().manual_seed(R + V)
            p = torch.softmax(torch.randn(R, V, generator=g) * 2.0, 1).to(torch.bfloat16).to(DEV)
            for name, (temp, k, pp, greedy) in (("greedy", (1.0, 0, 1.0, True)), ("sample", (1.0, 0, 1.0, False)),
                                                ("T.8 k50 p.9", (0.8, 50, 0.9, False))):
                ours = _med(lambda: GN.sample_rows_native(p, temp, k, pp, greedy, rng), passes, reps)
                if greedy:
                    ref = _med(lambda: torch.argmax(p, dim=1), passes, reps)
                elif k == 0 and pp == 1.0:
                    ref = _med(lambda: torch.multinomial(p.float(), 1), passes, reps)
                else:
                    ref = _med(lambda: _torch_sample(p, temp, k, pp), passes, reps)
                say(f"R={R:3d} V={V:6d} {name:12s}: kernel {ours[0]:8.1f} ({ours[1]:.1f} .. {ours[2]:.1f})   "
                    f"torch {ref[0]:8.1f} ({ref[1]:.1f} .. {ref[2]:.1f})   torch/kernel {ref[0] / ours[0]:5.2f}x")
    say()


def gather_mode(passes, reps):
    say(f"== cache gather per layer, bf16, C = 1536, capacity 256, GPU time per call in us (median of {passes} passes "
        f"of {reps})")
    for rows in (4, 128):
        for L in (128, 192):
            g = torch.Generator().manual_seed(rows + L)
            src = torch.randn(rows, 256, 1536, generator=g).to(torch.bfloat16).to(DEV)
            dst = torch.empty_like(src)
            par = torch.randint(0, rows, (rows,), generator=g).to(torch.int32).to(DEV)
            pl = par.long()
            ours = _med(lambda: GN.cache_gather_native(src, dst, par, L), passes, reps)
            ref = _med(lambda: src[:, :L].index_select(0, pl), passes, reps)
            nbytes = 2.0 * rows * L * 1536 * 2
            say(f"rows={rows:3d} L={L:3d}: kernel {ours[0]:7.1f} ({ours[1]:.1f} .. {ours[2]:.1f}) "
                f"{nbytes / ours[0] / 1e3:7.1f} GB/s   index_select {ref[0]:7.1f} ({ref[1]:.1f} .. {ref[2]:.1f})   "
                f"index_select/kernel {ref[0] / ours[0]:5.2f}x")
    say()


def _sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _user_loop(net, prompt, n, sample, eos):
    """The loop on the public API: fp32 output, torch ops for the choice, one host read per step."""
    net.rnnClearPreviousState()
    out = net.rnnTimeStep(prompt)[0]
    toks = []
    for _ in range(n):
        p = out[:, :, -1]
        t = torch.multinomial(p, 1) if sample else p.argmax(1, keepdim=True)
        toks.append(t)
        if bool((t == eos).all().item()):
            break
        out = net.rnnTimeStep(t)[0]
    return torch.cat(toks, 1)


def model_mode(batches, n, passes):
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, P = 77, 128
    net = TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=768, layers=12, heads=12, maxPositions=512,
                                    dataType=DataType.BFLOAT16).init(device=DEV)
    say(f"== generate() on TextGenerationTransformer(768, 12 layers, 12 heads), bf16, V = {V}, prefix {P}, {n} new "
        f"tokens, tokens/s (median of {passes}; min .. max); eos never met (token {V} does not exist)")
    say("   user loop = rnnTimeStep + argmax / torch.multinomial on the fp32 output + one .item() per step")
    for mb in batches:
        prompt = torch.randint(0, V, (mb, P), generator=torch.Generator().manual_seed(mb)).to(DEV)
        cases = (("greedy", dict(), False), ("sample", dict(doSample=True, seed=1), True),
                 ("T.8 k50 p.9", dict(doSample=True, temperature=0.8, topK=50, topP=0.9, seed=1), None),
                 ("numBeams=4", dict(numBeams=4), None))
        for name, kw, loop in cases:
            def ours():
                net.generate(prompt, maxNewTokens=n, **kw)
            ours()
            t = sorted(_sync_time(ours) for _ in range(passes))
            line = f"batch {mb:2d} {name:12s}: generate {mb * n / t[len(t) // 2]:9.1f} ({mb * n / t[-1]:.1f} .. " \
                   f"{mb * n / t[0]:.1f}) tok/s  {t[len(t) // 2] / n * 1e3:6.2f} ms/step"
            if loop is not None:
                _user_loop(net, prompt, n, loop, V)
                u = sorted(_sync_time(lambda: _user_loop(net, prompt, n, loop, V)) for _ in range(passes))
                line += f"   user loop {mb * n / u[len(u) // 2]:9.1f} ({mb * n / u[-1]:.1f} .. {mb * n / u[0]:.1f}) " \
                        f"tok/s   generate/loop {u[len(u) // 2] / t[len(t) // 2]:5.2f}x"
            say(line)
    say()


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sampler", action="store_true")
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        _out = open(a.out, "w")
    say(f"# tools/bench_generate.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if a.sampler:
        sampler_mode(a.passes, a.reps)
    if a.gather:
        gather_mode(a.passes, a.reps)
    if a.model:
        model_mode(a.batch, a.tokens, a.passes)


if __name__ == "__main__":
    main()
