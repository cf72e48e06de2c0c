#!/usr/bin/env python3
"""Measurements of the mixture-of-experts feed-forward (csrc/moe.hip, the grouped modes of csrc/gemm.hip) on one GPU.
Each mode writes its own section of profiles/moe.txt (a section is replaced when the mode runs again).

  python tools/bench_moe.py              the kernel rows below
  python tools/bench_moe.py --model      the 12-layer, hidden-768 rotary Llama-style model with nExperts = 8, k = 2,
                                         ffnSize 2048 against the dense model of ffnSize = k * 2048 (equal active
                                         parameters): tokens/s of generate() and generate(useGraph=True) at batch
                                         1 / 32 and prefix 128 / 1024, and a training step at batch 32 x 128
  DL4J_AMD_NATIVE=0 python tools/bench_moe.py --margin
                                         the router-logit difference between the 16-bit torch path and fp32 on the CPU
                                         on the model of tests/test_gpu_moe.py: the measurement behind its MARGIN

Kernel rows (bf16, E = 768, F = 2048, swiglu, X = 8, k = 2, 7 passes, median and spread between the passes):
  * the two grouped GEMMs at A = 8192 assignments, balanced and 4:1 skewed routing, against the dense ``mmul`` on 8192
    rows with the same K and N (equal FLOPs: the ratio is the cost of grouping);
  * the same at A = 64 (decode, batch 32) in bytes/s over the active experts' weights, against the two GEMMs of the
    dense feed-forward of ffnSize = k*F on 32 rows;
  * route + plan, gather and combine in TB/s, against the cache-gather copy (csrc/generation.hip) of the same bytes.
"""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "moe.txt")
E, F, X, K = 768, 2048, 8, 2
PASSES = 7


def _time(fn, iters=20):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(PASSES):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    med = statistics.median(out)
    return med, (max(out) - min(out)) / med * 100.0


def _logits(n, skew):
    import torch
    g = torch.Generator().manual_seed(n)
    l = torch.randn(n, X, generator=g)
    if skew:                                   # experts 0 and 1 take about 4x the tokens of the others
        l[:, :2] += 1.5
    return l.cuda()


def kernels():
    import torch
    from deeplearning4j_amd.ops import generation_native as GN
    from deeplearning4j_amd.ops import transformer_native as TN
    from deeplearning4j_amd.ops.gemm import mmul
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    w1 = (torch.randn(X, E, 2 * F, generator=g) * E ** -0.5).to(dt).to(dev)
    w2 = (torch.randn(X, F, E, generator=g) * F ** -0.5).to(dt).to(dev)
    rows = [f"bf16, E={E}, F={F}, swiglu (W1 [E, 2F]), X={X}, k={K}; {PASSES} passes of 20 calls, median (+- spread)"]
    for n, skew in ((4096, False), (4096, True), (32, False)):
        x = torch.randn(n, E, generator=g).to(dt).to(dev)
        lg = _logits(n, skew)
        plan, gate = TN.moe_route(lg, K)
        xp = TN.moe_gather(x, plan)
        z = TN.gemm_grouped(xp, w1, None, plan)
        f = TN.swiglu(z)
        y = TN.gemm_grouped(f, w2, None, plan)
        rows.append(f"A={n * K} {'skewed' if skew else 'balanced'}: cnt={plan.cnt.cpu().tolist()}, {plan.rows} rows")
        t1, s1 = _time(lambda: TN.gemm_grouped(xp, w1, None, plan, out=z))
        t2, s2 = _time(lambda: TN.gemm_grouped(f, w2, None, plan, out=y))
        if n > 32:
            xd, fd = xp[:n * K].contiguous(), f[:n * K].contiguous()
            d1, e1 = _time(lambda: mmul(xd, w1[0]))
            d2, e2 = _time(lambda: mmul(fd, w2[0]))
            rows.append(f"  grouped W1 {t1:8.1f} us (+-{s1:.1f}%)  dense mmul [{n * K}, {E}] x [{E}, {2 * F}] {d1:8.1f} us "
                        f"(+-{e1:.1f}%)  ratio {t1 / d1:.3f}")
            rows.append(f"  grouped W2 {t2:8.1f} us (+-{s2:.1f}%)  dense mmul [{n * K}, {F}] x [{F}, {E}] {d2:8.1f} us "
                        f"(+-{e2:.1f}%)  ratio {t2 / d2:.3f}")
        else:
            live = int((plan.cnt > 0).sum())
            b1, b2 = live * E * 2 * F * 2, live * F * E * 2
            wd1 = (torch.randn(E, 2 * K * F, generator=g) * E ** -0.5).to(dt).to(dev)     # dense FFN of ffnSize = k*F
            wd2 = (torch.randn(K * F, E, generator=g) * F ** -0.5).to(dt).to(dev)
            fd = torch.randn(n, K * F, generator=g).to(dt).to(dev)
            d1, e1 = _time(lambda: mmul(x, wd1))
            d2, e2 = _time(lambda: mmul(fd, wd2))
            rows.append(f"  grouped W1 {t1:8.1f} us (+-{s1:.1f}%) = {b1 / t1 / 1e6:.3f} TB/s over {live} active experts' "
                        f"weights; dense ffnSize=k*F [{n}, {E}] x [{E}, {2 * K * F}] {d1:8.1f} us (+-{e1:.1f}%) = "
                        f"{wd1.numel() * 2 / d1 / 1e6:.3f} TB/s")
            rows.append(f"  grouped W2 {t2:8.1f} us (+-{s2:.1f}%) = {b2 / t2 / 1e6:.3f} TB/s; dense [{n}, {K * F}] x "
                        f"[{K * F}, {E}] {d2:8.1f} us (+-{e2:.1f}%) = {wd2.numel() * 2 / d2 / 1e6:.3f} TB/s")
        tr, sr = _time(lambda: TN.moe_route(lg, K))
        tg, sg = _time(lambda: TN.moe_gather(x, plan, out=xp))
        tc, sc = _time(lambda: TN.moe_combine(y, plan, gate))
        a = n * K
        # the cache-gather copy of the same bytes: A rows of E values gathered by an index (read + write)
        src = x.reshape(n, 1, E)
        dst = torch.empty(a, 1, E, dtype=dt, device=dev)
        par = (torch.arange(a, device=dev, dtype=torch.int32) // K).contiguous()
        tk, sk = _time(lambda: GN.cache_gather_native(src, dst, par, 1))
        rows.append(f"  route+plan {tr:7.1f} us (+-{sr:.1f}%, 3 launches)")
        rows.append(f"  gather  {tg:7.1f} us = {2 * a * E * 2 / tg / 1e6:.3f} TB/s (+-{sg:.1f}%)   combine {tc:7.1f} us = "
                    f"{(a + n) * E * 2 / tc / 1e6:.3f} TB/s (+-{sc:.1f}%)   cache-gather copy of {a} rows {tk:7.1f} us = "
                    f"{2 * a * E * 2 / tk / 1e6:.3f} TB/s (+-{sk:.1f}%)")
    return rows


def _pass_times(fn, passes=PASSES):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    med = statistics.median(out)
    return med, (max(out) - min(out)) / med * 100.0


def model():
    import torch
    from deeplearning4j_amd import DataType
    from deeplearning4j_amd.models import TextGenerationTransformer
    dev, vocab, new = torch.device("cuda", 0), 1000, 32
    kw = dict(numLabels=vocab, inputShape=[128], hidden=E, layers=12, heads=12, maxPositions=2048, seed=1,
              dataType=DataType.BFLOAT16, positionEncoding="rotary", normalization="rms", normPlacement="pre",
              ffnActivation="swiglu")
    nets = {"moe X=8 k=2 ffn=2048": TextGenerationTransformer(ffn=F, nExperts=X, nExpertsPerToken=K, **kw),
            "dense ffn=4096": TextGenerationTransformer(ffn=K * F, **kw)}
    rows = [f"12 layers, hidden {E}, 12 heads, rotary, rms / pre / swiglu, bf16, V = {vocab}; {new} new tokens, greedy; "
            f"{PASSES} passes, median (+- spread)"]
    g = torch.Generator().manual_seed(0)
    for name, zoo in nets.items():
        net = zoo.init(device=dev)
        rows.append(f"{name}: {net.numParams() / 1e6:.1f} M parameters")
        for mb in (1, 32):
            for prefix in (128, 1024):
                prompt = torch.randint(0, vocab, (mb, prefix), generator=g).to(dev)
                for graph in (False, True):
                    t, sp = _pass_times(lambda: net.generate(prompt, maxNewTokens=new, useGraph=graph))
                    rows.append(f"  batch {mb:2d} prefix {prefix:4d} generate({'useGraph=True' if graph else ''}): "
                                f"{mb * new / t:9.0f} tokens/s, {t * 1e3:7.1f} ms per call (+-{sp:.1f}%)")
        x = torch.randint(0, vocab, (32, 128), generator=g).to(dev)
        y = torch.zeros(32, vocab, 128)
        y.scatter_(1, torch.randint(0, vocab, (32, 1, 128), generator=g), 1.0)
        y = y.to(dev)
        t, sp = _pass_times(lambda: net.fit([x], [y]))
        rows.append(f"  training step 32 x 128: {t * 1e3:7.1f} ms (+-{sp:.1f}%)")
        del net
        torch.cuda.empty_cache()
    return rows


# ---- the model of tests/test_gpu_moe.py (g), written out here so that the tool stands alone
V = 77
BLOCKS = ("decoder_0", "decoder_1")


def _lm(dt, device, seed):
    from deeplearning4j_amd.models import TextGenerationTransformer
    return TextGenerationTransformer(numLabels=V, hidden=128, layers=2, heads=2, nKVHeads=1, ffn=128, inputShape=[32],
                                     maxPositions=96, seed=seed, dataType=dt, positionEncoding="rotary",
                                     normalization="rms", normPlacement="pre", ffnActivation="swiglu", nExperts=4,
                                     nExpertsPerToken=2).init(device=device)


def _tokens(seed):
    import torch
    return torch.randint(0, 4, (3, 32), generator=torch.Generator().manual_seed(seed))


def _router_logits(net, x):
    import torch
    from deeplearning4j_amd.ops.gemm import mmul
    rec = []
    for name in BLOCKS:
        layer = net.layers_by_name[name]

        def fwd(n, acc=None, layer=layer, orig=layer._moe_fwd):
            sixteen = n.dtype in (torch.bfloat16, torch.float16)
            rec.append(mmul(n, layer.W("Wr"), out_dtype=torch.float32 if sixteen else None).float().cpu())
            return orig(n, acc)
        layer._moe_fwd = fwd
    net.output(x)
    for name in BLOCKS:
        del net.layers_by_name[name]._moe_fwd
    return rec


def _gap(logits, k=2):
    import torch
    s = torch.sort(logits, dim=1, descending=True).values
    return float((s[:, k - 1] - s[:, k]).min())


def margin():
    import torch
    from deeplearning4j_amd import DataType
    dev, worst = torch.device("cuda", 0), {}
    rows = ["model of tests/test_gpu_moe.py (g); max |logit(16-bit torch path, GPU) - logit(fp32 CPU)| over both blocks"]
    for seed in range(8):
        cpu = _lm(DataType.FLOAT, torch.device("cpu"), seed)
        ref = _router_logits(cpu, _tokens(seed))
        line = f"  seed {seed}"
        for name, dt in (("bf16", DataType.BFLOAT16), ("fp16", DataType.HALF)):
            gpu = _lm(dt, dev, seed)
            with torch.no_grad():
                gpu.flattenedParams.copy_(cpu.flattenedParams.to(dev))
            gpu._params_changed()
            got = _router_logits(gpu, _tokens(seed).to(dev))
            d = max(float((a - b).abs().max()) for a, b in zip(got, ref))
            worst[name] = max(worst.get(name, 0.0), d)
            line += f"  {name} {d:.3e}"
        rows.append(line + f"  smallest fp32 gap {min(_gap(l) for l in ref):.3e}")
    rows.append("  largest: " + ", ".join(f"{k_} {v:.3e}" for k_, v in worst.items()) + "; MARGIN = 8x = " +
                ", ".join(f"{k_} {8 * v:.3e}" for k_, v in worst.items()))
    return rows


def _write_section(title, rows):
    """Replace (or append) the section ``== title`` of profiles/moe.txt; a section ends at the next ``== `` line."""
    text = open(OUT).read() if os.path.exists(OUT) else ""
    body = f"== {title}\n" + "\n".join(rows) + "\n\n"
    pat = re.compile(rf"^== {re.escape(title)}\n.*?(?=^== |\Z)", re.S | re.M)
    text = pat.sub(lambda m: body, text) if pat.search(text) else text.rstrip("\n") + ("\n\n" if text else "") + body
    with open(OUT, "w") as fh:
        fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--margin", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--stdout", action="store_true", help="print only, leave profiles/moe.txt alone")
    args = ap.parse_args()
    if args.margin and os.environ.get("DL4J_AMD_NATIVE", "1") != "0":
        print("note: --margin measures the torch path; run it with DL4J_AMD_NATIVE=0", file=sys.stderr)
    if args.margin:
        title, rows = "tools/bench_moe.py --margin (DL4J_AMD_NATIVE=0)", margin()
    elif args.model:
        title, rows = "tools/bench_moe.py --model", model()
    else:
        title, rows = "tools/bench_moe.py (kernels)", kernels()
    print(f"== {title}\n" + "\n".join(rows))
    if not args.stdout:
        _write_section(title, rows)


if __name__ == "__main__":
    main()
