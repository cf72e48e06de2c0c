#!/usr/bin/env python3
"""Weight-only quantised decoding, the kernel alone (csrc/gemm_wq.hip): ``dl4j_wq_gemm`` in fp8 and fp4 against
``mmul`` on the 16-bit weights at the decode shapes of the 12-layer, hidden-768 model and a 32000-word vocabulary
projection, M = 1 and 32, bf16. GPU time per call by device events (ops.timing.gpu_time), the variants alternating
within every pass, median of the passes (min .. max); TB/s over the bytes a call reads (weights, scales, x, bias)
next to the rate of a device-to-device copy of 256 MiB measured in the same run.

--native: the skinny 16-bit kernel on the weights in place (csrc/gemm_skinny.hip, ``dl4j_skinny_gemm``) against ``mmul``
on the same weights, M = 1, 32 and 64, bf16 and fp16, next to the fp8 rows of the same run: the four block shapes
N-contiguous as the blocks hold them, with both load widths (4 / 8 columns per lane) and the kernel's rule, the
vocabulary projection K-contiguous as RnnOutputLayer holds it.

Usage: python tools/bench_wq.py [--native] [--passes 7] [--reps 50] [--out profiles/weight_quant.txt]"""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from deeplearning4j_amd.ops import transformer_native as TN  # noqa: E402
from deeplearning4j_amd.ops.gemm import mmul  # noqa: E402
from deeplearning4j_amd.ops.timing import gpu_time  # noqa: E402

DEV = torch.device("cuda", 0)
SHAPES = [(768, 2304), (768, 768), (768, 3072), (3072, 768), (768, 32000)]
_out = None


def say(s=""):
    print(s, flush=True)
    if _out is not None:
        _out.write(s + "\n")
        _out.flush()


def native(a):
    say(f"GPU time per call in us, median of {a.passes} passes of {a.reps} launches (min .. max), the variants "
        "alternating within a pass; bias in the epilogue; TB/s over the weight bytes; x = the 16-bit mmul's time over "
        "the variant's")
    for dt in (torch.bfloat16, torch.float16):
        for M in (1, 32, 64):
            for K, N in SHAPES:
                g = torch.Generator().manual_seed(K + N)
                W = (torch.randn(K, N, generator=g) * 0.05).to(dt).to(DEV)
                kcon = N == 32000
                if kcon:
                    W = W.t().contiguous().t()
                x = torch.randn(M, K, generator=g).to(dt).to(DEV)
                bias = torch.randn(N, generator=g).to(DEV)
                out = torch.empty(M, N, dtype=dt, device=DEV)
                q8 = TN.wq_quantize(W, "fp8")
                runs = [("16-bit mmul", lambda: mmul(x, W, out=out, bias=bias), 2 * K * N)]
                if kcon:
                    runs.append(("skinny K-contiguous", lambda: TN.skinny_gemm(x, W, bias, None, out), 2 * K * N))
                else:
                    runs += [(f"skinny width {wd or 'rule'}",
                              lambda wd=wd: TN.skinny_gemm(x, W, bias, None, out, width=wd), 2 * K * N)
                             for wd in (4, 8, 0)]
                runs.append(("fp8 wq_gemm", lambda: TN.wq_gemm(x, q8, bias, None, out),
                             q8.codes.numel() + q8.scales.numel()))
                for _, fn, _ in runs:
                    assert fn() is not None                         # the 16-bit product's autotuner, first launches
                times = [[] for _ in runs]
                for _ in range(a.passes):
                    for i, (_, fn, _) in enumerate(runs):
                        times[i].append(gpu_time(fn, reps=a.reps, warmup=3))
                med = [sorted(t)[len(t) // 2] for t in times]
                say(f"{str(dt).split('.')[1]}  M {M:2d}  K {K:5d}  N {N:5d}:")
                for (name, _, wb), t, m in zip(runs, times, med):
                    say(f"    {name:19s}: {m * 1e3:7.2f} us ({min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f})  "
                        f"{wb / m / 1e9:5.2f} TB/s  {med[0] / m:5.2f}x")
    say()


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--native", action="store_true", help="the skinny 16-bit kernel against mmul (see above)")
    a = ap.parse_args()
    if a.out:
        _out = open(a.out, "w")
    say(f"# tools/bench_wq.py{' --native' if a.native else ''} on {torch.cuda.get_device_name(0)}, "
        f"torch {torch.__version__}")
    if a.native:
        return native(a)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    t = sorted(gpu_time(lambda: dst.copy_(src), reps=20, warmup=3) for _ in range(a.passes))
    say(f"device copy of 256 MiB: {2 * src.numel() / t[len(t) // 2] / 1e9:.2f} TB/s read + written "
        f"({2 * src.numel() / t[-1] / 1e9:.2f} .. {2 * src.numel() / t[0] / 1e9:.2f})")
    say(f"GPU time per call in us, median of {a.passes} passes of {a.reps} launches (min .. max), the three variants "
        "alternating within a pass; bias in the epilogue; TB/s over the bytes read")
    for M in (1, 32):
        for K, N in SHAPES:
            g = torch.Generator().manual_seed(K + N)
            W = (torch.randn(K, N, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
            x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
            bias = torch.randn(N, generator=g).to(DEV)
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            q = {f: TN.wq_quantize(W, f) for f in ("fp8", "fp4")}
            runs = [("16-bit mmul", lambda: mmul(x, W, out=out, bias=bias), 2 * K * N),
                    ("fp8 wq_gemm", lambda: TN.wq_gemm(x, q["fp8"], bias, None, out), q["fp8"].codes.numel() +
                     q["fp8"].scales.numel()),
                    ("fp4 wq_gemm", lambda: TN.wq_gemm(x, q["fp4"], bias, None, out), q["fp4"].codes.numel() +
                     q["fp4"].scales.numel())]
            for _, fn, _ in runs:
                fn()                                            # the 16-bit product's autotuner, first launches
            times = [[] for _ in runs]
            for _ in range(a.passes):
                for i, (_, fn, _) in enumerate(runs):
                    times[i].append(gpu_time(fn, reps=a.reps, warmup=3))
            med = [sorted(t)[len(t) // 2] for t in times]
            say(f"M {M:2d}  K {K:5d}  N {N:5d}:")
            for (name, _, wb), t, m in zip(runs, times, med):
                nbytes = wb + 2 * M * K + 4 * N
                say(f"    {name}: {m * 1e3:7.2f} us ({min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f})  {nbytes / 1e6:7.2f} MB "
                    f"read  {nbytes / m / 1e9:5.2f} TB/s  {med[0] / m:5.2f}x the 16-bit product")
    say()


if __name__ == "__main__":
    main()
