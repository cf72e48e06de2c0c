#!/usr/bin/env python3
"""RMSNorm and SwiGLU kernel timings (csrc/rmsnorm.hip, csrc/swiglu.hip), bf16, GPU-side time (ops/timing.gpu_time).

  norms    dl4j_rms_fwd / dl4j_rms_bwd against dl4j_ln_fwd / dl4j_ln_bwd of this tree on the same operands, with a
           residual and the column sums of dx, M = 4096 rows at N = 768 and N = 4096. The entry points are called
           directly on buffers allocated once; the four alternate within every pass. Bytes: the operands each call
           must read and write once (forward x, r, y (+ s for RMSNorm); backward dy, s (x, r for LayerNorm), dres, dx).
  swiglu   dl4j_swiglu_fwd / dl4j_swiglu_bwd as achieved bytes per second (forward 2F in + F out, backward 3F in +
           2F out, per row) at M = 4096 with F = 3072 and F = 11008, next to the cache-gather copy kernel on a buffer
           of the forward's bytes (the tree's copy yardstick, profiles/generation.txt).

Usage: python tools/bench_norm.py [--passes 7] [--reps 50] [--out profiles/llama_block.txt]"""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from deeplearning4j_amd.ops import generation_native as GN  # noqa: E402
from deeplearning4j_amd.ops import native  # noqa: E402
from deeplearning4j_amd.ops.native import _ptr, _stream  # noqa: E402
from deeplearning4j_amd.ops.timing import gpu_time  # noqa: E402

DEV = torch.device("cuda", 0)
_out = None


def say(s=""):
    print(s, flush=True)
    if _out is not None:
        _out.write(s + "\n")
        _out.flush()


def _passes(fns, passes, reps):
    """{name: sorted microseconds per call}, the functions alternating within every pass."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(passes):
        for k, fn in fns.items():
            t[k].append(gpu_time(fn, reps=reps) * 1e3)
    return {k: sorted(v) for k, v in t.items()}


def _row(name, t, nbytes, base=None):
    med = t[len(t) // 2]
    rel = "" if base is None else f"  x {base / med:5.3f}"
    say(f"{name:28s} {med:8.1f} us ({t[0]:.1f} .. {t[-1]:.1f})  {nbytes / med * 1e-6:6.2f} TB/s{rel}")


def norms(passes, reps):
    L = native.load()
    s = _stream()
    say(f"== RMSNorm against LayerNorm, bf16, M = 4096, with a residual; backward with the column sums of dx; median of "
        f"{passes} passes of {reps} calls (min .. max), the kernels alternating within a pass; x = LayerNorm's time "
        "over RMSNorm's")
    for N in (768, 4096):
        M = 4096
        g = torch.Generator().manual_seed(N)
        mk = lambda: torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)  # noqa: E731
        x, r, dy, dres = mk(), mk(), mk(), mk()
        y, so, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        gamma, beta = (torch.rand(N, generator=g) + 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
        mean, rstd, rstd2 = (torch.empty(M, device=DEV) for _ in range(3))
        dg, db, dsum = (torch.empty(N, device=DEV) for _ in range(3))
        part = torch.empty(max(L.dl4j_ln_partial_rows(M) * 3, L.dl4j_rms_partial_rows(M) * 2) * N, device=DEV)
        fns = {
            "ln_fwd": lambda: L.dl4j_ln_fwd(1, _ptr(x), _ptr(r), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean),
                                            _ptr(rstd), M, N, 1e-5, s),
            "rms_fwd": lambda: L.dl4j_rms_fwd(1, _ptr(x), _ptr(r), _ptr(gamma), _ptr(y), _ptr(so), _ptr(rstd2), M, N,
                                              1e-5, s),
            "ln_bwd": lambda: L.dl4j_ln_bwd(1, _ptr(dy), _ptr(x), _ptr(r), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx),
                                            _ptr(part), _ptr(dg), _ptr(db), _ptr(dsum), M, N, s),
            "rms_bwd": lambda: L.dl4j_rms_bwd(1, _ptr(dy), _ptr(so), _ptr(gamma), _ptr(rstd2), _ptr(dres), _ptr(dx),
                                              _ptr(part), _ptr(dg), _ptr(dsum), M, N, s),
        }
        for k, fn in fns.items():
            assert fn() == 0, k
        t = _passes(fns, passes, reps)
        e = 2 * M * N
        say(f"-- N = {N}")
        _row("ln_fwd  (x, r -> y)", t["ln_fwd"], 3 * e)
        _row("rms_fwd (x, r -> s, y)", t["rms_fwd"], 4 * e, t["ln_fwd"][len(t["ln_fwd"]) // 2])
        _row("ln_bwd  (dy, x, r -> dx)", t["ln_bwd"], 4 * e)
        _row("rms_bwd (dy, s, dres -> dx)", t["rms_bwd"], 4 * e, t["ln_bwd"][len(t["ln_bwd"]) // 2])
    say()


def swiglu(passes, reps):
    L = native.load()
    s = _stream()
    say(f"== SwiGLU, bf16, M = 4096: achieved bytes per second (forward 2F in + F out, backward 3F in + 2F out per row) "
        f"next to the cache-gather copy kernel moving the forward's bytes; median of {passes} passes of {reps} calls "
        "(min .. max), alternating within a pass; x = the copy's bytes per second over the kernel's")
    for F_ in (3072, 11008):
        M = 4096
        g = torch.Generator().manual_seed(F_)
        gu = (torch.randn(M, 2 * F_, generator=g) * 3).to(torch.bfloat16).to(DEV)
        df = torch.randn(M, F_, generator=g).to(torch.bfloat16).to(DEV)
        out, dgu = torch.empty_like(df), torch.empty_like(gu)
        # the copy yardstick: gather M rows of 3F/2 elements from a cache of one valid row each (reads + writes 3F*M)
        src = torch.randn(M, 1, 3 * F_ // 2, generator=g).to(torch.bfloat16).to(DEV)
        dst = torch.empty_like(src)
        parents = torch.arange(M, dtype=torch.int32, device=DEV)
        fns = {
            "fwd": lambda: L.dl4j_swiglu_fwd(1, _ptr(gu), _ptr(out), M, F_, s),
            "bwd": lambda: L.dl4j_swiglu_bwd(1, _ptr(gu), _ptr(df), _ptr(dgu), M, F_, s),
            "copy": lambda: GN.cache_gather(src, dst, parents, 1),
        }
        assert fns["fwd"]() == 0 and fns["bwd"]() == 0
        t = _passes(fns, passes, reps)
        e = 2 * M * F_
        bps = {"fwd": 3 * e, "bwd": 5 * e, "copy": 3 * e}
        copy_rate = bps["copy"] / t["copy"][len(t["copy"]) // 2]
        say(f"-- F = {F_}")
        for k in ("copy", "fwd", "bwd"):
            med = t[k][len(t[k]) // 2]
            rel = "" if k == "copy" else f"  x {copy_rate / (bps[k] / med):5.3f}"
            say(f"{k:5s} {med:8.1f} us ({t[k][0]:.1f} .. {t[k][-1]:.1f})  {bps[k] / med * 1e-6:6.2f} TB/s{rel}")
    say()


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        _out = open(a.out, "a")
    say(f"# tools/bench_norm.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    norms(a.passes, a.reps)
    swiglu(a.passes, a.reps)


if __name__ == "__main__":
    main()
