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
  --ragged   ragged prompts (per-row cache lengths). (a) the decode-attention kernel with an all-zero shortfall array
             against the uniform kernel on the same operands, at the shapes of profiles/decode_attention.txt, the
             variants alternating within every pass; with --parent-lib also against the uniform kernel of a kernel
             library built from the parent commit. (b) generate(promptLengths=...) on 32 prompts with lengths spread
             evenly over [Tp/4, Tp] against the same prompts generated one length bucket at a time (rows grouped by
             their exact length, one generate() per group), same model as --model; the tokens of both are compared.

  --graph    graph-replayed decoding: generate(useGraph=True) against generate() (useGraph=False) on the same network in
             the same process, the two alternating within every pass; with --parent-lib also against generate() with
             every kernel call going to a kernel library built from the parent commit. 12-layer, hidden-768 model at
             batch 1 / 32, prefix 128 / 1024, greedy and temperature 0.8 / top-k 50 / top-p 0.9; the 32-prompt ragged
             batch of --ragged; TransformerSeq2Seq (hidden 768, 6 + 6 layers, source 128) at batch 1. Also the
             one-off cost of a graph call (its warm-up step and the capture) and the maxNewTokens from which the
             graph call is the faster one.

  --cache fp8  generate() and generate(useGraph=True) with the fp8 key/value cache against the 16-bit cache on one
             network (rnnSetCacheDataType switches it between the calls), the four variants alternating within every
             pass: 12-layer, hidden-768 model with maxPositions 4096 at the batch sizes of --batch (default 32),
             prefix 1024 and the longest prefix that leaves room for the new tokens; also the cache bytes per layer.

  --kv-heads N[,N..]  grouped-query attention: generate() and generate(useGraph=True) of the 12-layer, hidden-768
             model built with nKVHeads = N against the 12-head model (one network per count), prefix 1024, the
             variants alternating within every pass; also the cache bytes per cached token and layer.

  --rotary   rotary position embeddings: generate() and generate(useGraph=True) of the 12-layer, hidden-768 model
             built with positionEncoding="rotary" against the same model with learned positions (one network each),
             prefix 128 and 1024, the variants alternating within every pass; then one causal-LM training step
             (batch 32, 128 tokens) of both. ``--positions learned`` measures the learned-position model alone and
             ``--tree PATH`` imports the package from another checkout (the parent commit's, with its own kernel
             library), so the same rows can be taken from both trees in alternating processes.

  --block llama  Llama-style blocks (RMSNorm, pre-norm, SwiGLU with ffnSize 2048) against post-LayerNorm GELU blocks
             (ffnSize 3072, the same parameter count) on the rotary 12-layer, hidden-768 model: the rows of --rotary.

  --window W  sliding-window attention (attentionWindow = W in every block) against none on the rotary 12-layer,
             hidden-768 model: generate() and generate(useGraph=True) at prefix 1024 and 4032, and a causal-LM
             training step of batch 32 at 2048 tokens.

  --speculative K[,K..] [--draft-layers L | --lookup]  speculative decoding: the verify / commit / n-gram draft
             kernels alone at V in {77, 32000, 128000}; then generate(numDraftTokens=K) against generate() on the
             12-layer, hidden-768 model (prefix 128), drafts from an L-layer assistant of the same width (default 2) or
             from prompt lookup, the variants alternating within every pass: time per round and per plain step, the
             acceptance observed (random weights: no statement about trained models) and the break-even acceptance.
             With ``--model --tree PATH`` the plain generate() rows can be taken from the parent commit's checkout.

Usage: python tools/bench_generate.py --sampler --gather --model [--out profiles/generation.txt]
       python tools/bench_generate.py --speculative 2,4,8 [--lookup] [--out profiles/speculative.txt]
       python tools/bench_generate.py --ragged [--parent-lib PATH] [--out profiles/ragged_generation.txt]
       python tools/bench_generate.py --graph [--parent-lib PATH] [--out profiles/generation_graph.txt]
       python tools/bench_generate.py --cache fp8 [--batch 32] [--out FILE]
       python tools/bench_generate.py --kv-heads 4 [--batch 32] [--out FILE]
       python tools/bench_generate.py --rotary [--positions learned] [--tree PATH] [--out FILE]
       python tools/bench_generate.py --block llama [--out FILE]
       python tools/bench_generate.py --window 256 --batch 32 [--out FILE]"""
import argparse
import sys
import time

import torch

# --tree PATH: the checkout the package is imported from (default: this one)
sys.path.insert(0, sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv[:-1]
                else __file__.rsplit("/tools/", 1)[0])
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


def _decode_call(lib, qkv, kv, out, ws, short, B, H, D, pos, splits):
    """One decode-attention launch straight on a kernel library's C ABI (the uniform entry point when ``short`` is
    None); argument types set by hand so that a library without the ragged entry point can be driven too."""
    import ctypes
    vp, ci = ctypes.c_void_p, ctypes.c_int
    ptr = lambda t: None if t is None else vp(t.data_ptr())      # noqa: E731
    stream = vp(torch.cuda.current_stream().cuda_stream)
    scale = ctypes.c_float(D ** -0.5)
    if short is None:
        f = lib.dl4j_attn_decode_dt
        f.argtypes = [ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.c_float, vp]
        return f(1, ptr(qkv), ptr(kv), ptr(out), ptr(ws), B, 1, H, D, pos, kv.shape[1], splits, scale, stream)
    f = lib.dl4j_attn_decode_ragged_dt
    f.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.c_float, vp]
    return f(1, ptr(qkv), ptr(kv), ptr(out), ptr(ws), ptr(short), B, 1, H, D, pos, kv.shape[1], splits, scale, stream)


def ragged_kernel_mode(passes, reps, parent_lib):
    import ctypes
    from deeplearning4j_amd.ops import native
    from deeplearning4j_amd.ops import transformer_native as TN
    libs = [("uniform", ctypes.CDLL(native.KERNEL_LIB), False), ("zero shortfall", ctypes.CDLL(native.KERNEL_LIB), True)]
    if parent_lib:
        libs.insert(0, ("parent uniform", ctypes.CDLL(parent_lib), False))
    say(f"== attn_decode, Tn = 1, bf16, default splits, GPU time per call in us (mean of {reps} back-to-back launches; "
        f"median of {passes} passes, min .. max; the variants alternate within a pass)")
    say("   uniform = this tree's kernel without an array; zero shortfall = the ragged kernel with an all-zero array"
        + ("; parent uniform = the parent commit's kernel library" if parent_lib else ""))
    H, D = 12, 64
    E = H * D
    for B in (1, 32):
        for L in (128, 1024, 4096):
            torch.manual_seed(B + L)
            pos = L - 1
            qkv = (torch.randn(B, 1, 3 * E, device=DEV) * 0.8).to(torch.bfloat16)
            kv = (torch.randn(B, L + 64, 2 * E, device=DEV) * 0.8).to(torch.bfloat16)
            short = torch.zeros(B, dtype=torch.int32, device=DEV)
            splits = TN.attn_decode_splits(B, 1, H, D, L)
            ws = torch.empty(max(1, B * H * splits * (D + 2)), dtype=torch.float32, device=DEV)
            outs, times = [], [[] for _ in libs]
            for _, lib, rag in libs:
                o = torch.empty(B, 1, E, dtype=torch.bfloat16, device=DEV)
                assert _decode_call(lib, qkv, kv, o, ws, short if rag else None, B, H, D, pos, splits) == 0
                outs.append(o)
            torch.cuda.synchronize()
            same = all(torch.equal(outs[0], o) for o in outs[1:])
            for _ in range(passes):
                for i, (_, lib, rag) in enumerate(libs):
                    o = outs[i]
                    times[i].append(gpu_time(lambda: _decode_call(lib, qkv, kv, o, ws, short if rag else None, B, H,
                                                                  D, pos, splits), reps=reps, warmup=3) * 1e3)
            line = f"B={B:2d} H={H} D={D} L={L:4d} splits={splits:2d}:"
            med = []
            for (name, _, _), t in zip(libs, times):
                t = sorted(t)
                med.append(t[len(t) // 2])
                line += f"  {name} {t[len(t) // 2]:7.2f} ({t[0]:.2f} .. {t[-1]:.2f})"
            line += f"  zero shortfall / uniform {med[-1] / med[-2]:5.3f}x"
            if parent_lib:
                line += f"  uniform / parent {med[1] / med[0]:5.3f}x"
            say(line + f"  outputs bitwise equal: {same}")
    say()


def ragged_model_mode(n, passes):
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, Tp, mb = 77, 128, 32
    net = TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=768, layers=12, heads=12, maxPositions=512,
                                    dataType=DataType.BFLOAT16).init(device=DEV)
    g = torch.Generator().manual_seed(mb)
    lens = [Tp // 4 + (b * (Tp - Tp // 4)) // (mb - 1) for b in range(mb)]          # 32 .. 128, evenly spread
    prompt = torch.randint(0, V, (mb, Tp), generator=g)
    for b, L in enumerate(lens):
        prompt[b, L:] = 0
    prompt = prompt.to(DEV)
    buckets = {}
    for b, L in enumerate(lens):
        buckets.setdefault(L, []).append(b)
    parts = [(torch.tensor(rows, device=DEV), prompt[rows, :L].contiguous()) for L, rows in sorted(buckets.items())]
    say(f"== generate() on TextGenerationTransformer(768, 12 layers, 12 heads), bf16, V = {V}, greedy, {n} new tokens, "
        f"{mb} prompts of lengths {lens[0]} .. {lens[-1]} ({len(buckets)} distinct), tokens/s (median of {passes}; "
        "min .. max), host clock around work that ends in a device synchronise")
    say(f"   ragged = one generate(promptLengths=...) on the [32, {Tp}] right-padded batch; bucketed = one generate() "
        "per distinct length on the rows of that length, unpadded; same batch = one generate() on 32 full-length "
        "prompts (no lengths), the cost of the batch without raggedness")

    def ragged():
        return net.generate(prompt, promptLengths=lens, maxNewTokens=n)

    def bucketed():
        toks = torch.empty(mb, n, dtype=torch.int64, device=DEV)
        for rows, p in parts:
            toks[rows] = net.generate(p, maxNewTokens=n).tokens
        return toks

    def full():
        return net.generate(prompt, maxNewTokens=n)

    a, b = ragged().tokens, bucketed()
    full()
    agree = (a == b).all(1).float().mean().item()
    say(f"   rows whose {n} tokens are the same in both: {agree * 100:.1f} % (bf16: batch-size dependent GEMM kernels "
        "may flip near-ties)")
    tr, tb, tf = [], [], []
    for _ in range(passes):
        tr.append(_sync_time(ragged))
        tb.append(_sync_time(bucketed))
        tf.append(_sync_time(full))
    tr, tb, tf = sorted(tr), sorted(tb), sorted(tf)
    m = passes // 2
    for name, t in (("ragged", tr), ("bucketed", tb), ("same batch, no lengths", tf)):
        say(f"{name:24s}: {mb * n / t[m]:9.1f} ({mb * n / t[-1]:.1f} .. {mb * n / t[0]:.1f}) tok/s  "
            f"{t[m] * 1e3:8.1f} ms per batch")
    say(f"bucketed / ragged time: {tb[m] / tr[m]:5.2f}x   ragged / same batch time: {tr[m] / tf[m]:5.3f}x")
    say()


def _parent_library(path):
    """The parent commit's kernel library with the signatures of the entry points it has (it lacks the new ones)."""
    import ctypes
    from deeplearning4j_amd.ops import abi
    lib = ctypes.CDLL(path)
    for name, (args, res) in abi.signatures().items():
        f = getattr(lib, name, None) if name.startswith("dl4j_") else None
        if f is not None:
            f.argtypes, f.restype = args, res
    return lib


def _graph_case(name, call, n, rows, passes, parent):
    """``call(**kw)`` runs one generate(); kw selects the variant. The variants alternate within a pass."""
    import contextlib
    from deeplearning4j_amd.ops import native

    @contextlib.contextmanager
    def through(lib):
        ours, native._lib = native._lib, lib
        try:
            yield
        finally:
            native._lib = ours

    def eager():
        return call()

    def graph():
        return call(useGraph=True)

    def pinned():
        return call(pinPositions=True)

    def par():
        with through(parent):
            return call()

    variants = [("eager", eager), ("graph", graph), ("pinned eager", pinned)] + ([("parent", par)] if parent else [])
    outs = [fn() for _, fn in variants]
    same = [bool((o.tokens == outs[0].tokens).all()) for o in outs]
    times = [[] for _ in variants]
    for _ in range(passes):
        for i, (_, fn) in enumerate(variants):
            times[i].append(_sync_time(fn))
    med = [sorted(t)[len(t) // 2] for t in times]
    # the one-off cost and the steady step of a graph call: a call's time is a + b * tokens, so time it at 3n too
    long_n = 3 * n
    tl = sorted(_sync_time(lambda: call(useGraph=True, maxNewTokens=long_n)) for _ in range(passes))[passes // 2]
    el = sorted(_sync_time(lambda: call(maxNewTokens=long_n)) for _ in range(passes))[passes // 2]
    gstep, estep = (tl - med[1]) / (long_n - n), (el - med[0]) / (long_n - n)
    once = (med[1] - n * gstep) - (med[0] - n * estep)            # what a graph call pays on top, once
    even = "never" if gstep >= estep else f"{max(1, int(once / (estep - gstep)) + 1)}"
    line = f"{name:34s}:"
    for (vn, _), t, m in zip(variants, times, med):
        line += f"  {vn} {rows * n / m:8.1f} tok/s {m / n * 1e3:5.2f} ms/tok " \
                f"({min(t) * 1e3:.0f} .. {max(t) * 1e3:.0f} ms)"
    line += f"  graph/eager {med[0] / med[1]:5.2f}x"
    if parent:
        line += f"  graph/parent {med[3] / med[1]:5.2f}x  eager/parent {med[3] / med[0]:5.3f}x"
    say(line)
    say(f"{'':34s}   from the same calls with {long_n} tokens: replayed step {gstep * 1e3:5.2f} ms vs eager step "
        f"{estep * 1e3:5.2f} ms; warm-up + capture "
        f"{once * 1e3:6.1f} ms per call; graph call faster from maxNewTokens = {even}; tokens equal to eager's: "
        + ", ".join(f"{vn} {ok}" for (vn, _), ok in zip(variants[1:], same[1:])))


def graph_mode(batches, n, passes, parent_lib):
    from deeplearning4j_amd.models import TextGenerationTransformer, TransformerSeq2Seq
    from deeplearning4j_amd.nn.conf import DataType
    V = 77
    parent = _parent_library(parent_lib) if parent_lib else None
    net = TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=768, layers=12, heads=12, maxPositions=2048,
                                    dataType=DataType.BFLOAT16).init(device=DEV)
    say(f"== generate(useGraph=True) against generate() on TextGenerationTransformer(768, 12 layers, 12 heads), bf16, "
        f"V = {V}, {n} new tokens; whole calls (prompt included) on the host clock, ended by a device synchronise; "
        f"median of {passes} passes (min .. max), the variants alternating within a pass")
    say("   eager = useGraph=False; graph = one eager step, one capture, replays; pinned eager = pinPositions=True "
        "(the graph call's launches, not captured)"
        + ("; parent = eager with every kernel call going to the parent commit's kernel library" if parent else ""))
    say("   one bound for the whole call: every step launches the split count of the final length")
    sampling = dict(doSample=True, temperature=0.8, topK=50, topP=0.9, seed=1)
    for mb in batches:
        for P in (128, 1024):
            prompt = torch.randint(0, V, (mb, P), generator=torch.Generator().manual_seed(mb + P)).to(DEV)
            for cname, kw in (("greedy", dict()), ("T.8 k50 p.9", sampling)):
                def call(prompt=prompt, kw=kw, **over):
                    return net.generate(prompt, **dict(dict(kw, maxNewTokens=n), **over))
                _graph_case(f"batch {mb:2d} prefix {P:4d} {cname}", call, n, mb, passes, parent)
    mb, Tp = 32, 128
    lens = [Tp // 4 + (b * (Tp - Tp // 4)) // (mb - 1) for b in range(mb)]
    prompt = torch.randint(0, V, (mb, Tp), generator=torch.Generator().manual_seed(mb)).to(DEV)

    def ragged(**over):
        return net.generate(prompt, promptLengths=lens, **dict(dict(maxNewTokens=n), **over))
    _graph_case(f"32 ragged prompts {lens[0]}..{lens[-1]} greedy", ragged, n, mb, passes, parent)
    del net
    s2s = TransformerSeq2Seq(numLabels=V, inputShape=[128, 128], hidden=768, layers=6, heads=12, maxPositions=512,
                             dataType=DataType.BFLOAT16).init(device=DEV)
    src = torch.randint(0, V, (1, 128), generator=torch.Generator().manual_seed(5)).to(DEV)
    start = torch.zeros(1, 1, dtype=torch.int64, device=DEV)

    def seq2seq(**over):
        return TransformerSeq2Seq.generate(s2s, src, start, **dict(dict(maxNewTokens=n), **over))
    _graph_case("TransformerSeq2Seq 6+6 batch 1 greedy", seq2seq, n, 1, passes, parent)
    say()


def cache_fp8_mode(batches, n, passes):
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    from deeplearning4j_amd.ops import transformer_native as TN
    V, MAXP, H, E = 77, 4096, 12, 768
    net = TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=E, layers=12, heads=H, maxPositions=MAXP,
                                    dataType=DataType.BFLOAT16).init(device=DEV)
    R = TN.kv_fp8_row_bytes(H, E // H)
    say(f"== generate() with the fp8 key/value cache against the 16-bit cache on TextGenerationTransformer(768, 12 "
        f"layers, 12 heads, maxPositions {MAXP}), bf16, V = {V}, greedy, {n} new tokens; whole calls (prompt included) "
        f"on the host clock, ended by a device synchronise; median of {passes} passes (min .. max), the variants "
        "alternating within a pass; one network, rnnSetCacheDataType between the calls")
    say(f"   cache bytes per cached token and layer: 16-bit {4 * E}, fp8 {R} ({R / (4 * E):.3f})")

    def call(prompt, cache, **kw):
        net.rnnClearPreviousState()
        net.rnnSetCacheDataType(cache)
        return net.generate(prompt, maxNewTokens=n, **kw)

    for mb in batches:
        for P in (1024, MAXP - n):
            prompt = torch.randint(0, V, (mb, P), generator=torch.Generator().manual_seed(mb + P)).to(DEV)
            variants = [("16-bit eager", None, {}), ("fp8 eager", "fp8", {}),
                        ("16-bit graph", None, dict(useGraph=True)), ("fp8 graph", "fp8", dict(useGraph=True))]
            outs, held = [], []
            for _, cache, kw in variants:
                outs.append(call(prompt, cache, **kw).tokens)
                kv = net.layers_by_name["decoder_0"]._kv
                held.append(kv.numel() * kv.element_size())
            agree = [(o == outs[0]).float().mean().item() for o in outs]
            times = [[] for _ in variants]
            for _ in range(passes):
                for i, (_, cache, kw) in enumerate(variants):
                    times[i].append(_sync_time(lambda: call(prompt, cache, **kw)))
            med = [sorted(t)[len(t) // 2] for t in times]
            say(f"batch {mb:2d} prefix {P:4d}: valid cache per layer 16-bit {mb * (P + n) * 4 * E / 1e6:7.1f} MB, fp8 "
                f"{mb * (P + n) * R / 1e6:7.1f} MB; allocated per layer after the call "
                + ", ".join(f"{vn} {b / 1e6:.1f} MB" for (vn, _, _), b in zip(variants, held)))
            for (vn, _, _), t, m, ag in zip(variants, times, med, agree):
                say(f"    {vn:13s}: {mb * n / m:9.1f} tok/s  {m * 1e3:8.1f} ms per call ({min(t) * 1e3:.1f} .. "
                    f"{max(t) * 1e3:.1f})  tokens equal to 16-bit eager's: {ag * 100:5.1f} %")
            say(f"    fp8 / 16-bit tokens/s: eager {med[0] / med[1]:5.3f}x  graph {med[2] / med[3]:5.3f}x   "
                f"(whole calls: the prompt's forward is in both)")
            # the steady step alone: a call's time is a + b * tokens, so time n / 4 tokens too
            few = max(2, n // 4)
            short = []
            for _, cache, kw in variants:
                net.rnnClearPreviousState()
                net.rnnSetCacheDataType(cache)
                fn = lambda: net.generate(prompt, maxNewTokens=few, **kw)              # noqa: E731
                fn()
                short.append(sorted(_sync_time(fn) for _ in range(passes))[passes // 2])
            per = [(m - ts) / (n - few) * 1e3 for ts, m in zip(short, med)]
            say(f"    step alone (against the same calls with {few} tokens): "
                + ", ".join(f"{vn} {v:5.2f} ms" for (vn, _, _), v in zip(variants, per))
                + f"; 16-bit / fp8 step time: eager {per[0] / per[1]:5.3f}x  graph {per[2] / per[3]:5.3f}x")
    net.rnnClearPreviousState()
    net.rnnSetCacheDataType(None)
    say()


def kv_heads_mode(kv_heads, batches, n, passes):
    """generate() and generate(useGraph=True) of the 12-layer, hidden-768 model with nKVHeads key/value heads against
    the 12-head model: one network per head count (the projection shapes differ), the variants alternating."""
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, MAXP, H, E, P = 77, 2048, 12, 768, 1024
    D = E // H
    heads = [H] + [h for h in kv_heads if h != H]
    nets = {h: TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=E, layers=12, heads=H, nKVHeads=h,
                                         maxPositions=MAXP, dataType=DataType.BFLOAT16).init(device=DEV) for h in heads}
    say(f"== generate() with grouped key/value heads on TextGenerationTransformer(768, 12 layers, 12 query heads, "
        f"maxPositions {MAXP}), bf16, V = {V}, greedy, prefix {P}, {n} new tokens; whole calls (prompt included) on "
        f"the host clock, ended by a device synchronise; median of {passes} passes (min .. max), the variants alternating "
        "within a pass; x = tokens/s against the 12-head model's same mode")
    say("   16-bit cache bytes per cached token and layer: "
        + ", ".join(f"nKVHeads {h}: {4 * h * D} ({h / H:.3f})" for h in heads)
        + "; parameters: " + ", ".join(f"nKVHeads {h}: {nets[h].numParams()}" for h in heads))
    for mb in batches:
        prompt = torch.randint(0, V, (mb, P), generator=torch.Generator().manual_seed(mb + P)).to(DEV)
        variants = [(f"nKVHeads {h:2d} {mode}", nets[h], kw)
                    for mode, kw in (("eager", {}), ("graph", dict(useGraph=True))) for h in heads]

        def call(net, kw, tokens=n):
            net.rnnClearPreviousState()
            return net.generate(prompt, maxNewTokens=tokens, **kw)

        for _, net, kw in variants:
            call(net, kw)
        times = [[] for _ in variants]
        for _ in range(passes):
            for i, (_, net, kw) in enumerate(variants):
                times[i].append(_sync_time(lambda: call(net, kw)))
        med = [sorted(t)[len(t) // 2] for t in times]
        few = max(2, n // 4)
        short = []
        for _, net, kw in variants:
            call(net, kw, few)
            short.append(sorted(_sync_time(lambda: call(net, kw, few)) for _ in range(passes))[passes // 2])
        per = [(m - ts) / (n - few) * 1e3 for ts, m in zip(short, med)]
        for i, ((vn, _, _), t, m) in enumerate(zip(variants, times, med)):
            b = (i // len(heads)) * len(heads)                   # the 12-head row of the same mode
            say(f"batch {mb:2d} {vn}: {mb * n / m:9.1f} tok/s  {m * 1e3:8.1f} ms per call ({min(t) * 1e3:.1f} .. "
                f"{max(t) * 1e3:.1f})  x {med[b] / m:5.3f} | step alone {per[i]:6.2f} ms  x {per[b] / per[i]:5.3f}")
    for net in nets.values():
        net.rnnClearPreviousState()
    say()


def rotary_mode(batches, n, passes, positions):
    """generate() / generate(useGraph=True) and a training step of the 12-layer, hidden-768 model with rotary
    embeddings against learned positions: one network each, the variants alternating."""
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, MAXP, H, E = 77, 2048, 12, 768
    kinds = ["learned", "rotary"] if positions == "both" else [positions]
    nets = {k: TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=E, layers=12, heads=H, maxPositions=MAXP,
                                         dataType=DataType.BFLOAT16,
                                         **(dict(positionEncoding="rotary") if k == "rotary" else {})).init(device=DEV)
            for k in kinds}
    say(f"== generate() with rotary embeddings against learned positions on TextGenerationTransformer(768, 12 layers, "
        f"12 heads, maxPositions {MAXP}), bf16, V = {V}, greedy, {n} new tokens; whole calls (prompt included) on the "
        f"host clock, ended by a device synchronise; median of {passes} passes (min .. max), the variants alternating "
        "within a pass; x = tokens/s against the learned-position model's same mode")
    _compare_models(nets, kinds, V, batches, n, passes)


def block_mode(batches, n, passes):
    """--block llama: the Llama-style block (RMSNorm, pre-norm, SwiGLU with ffnSize 2048) against today's (LayerNorm,
    post-norm, GELU with ffnSize 3072) at equal parameter count on the 12-layer, hidden-768 rotary model."""
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, H, E = 77, 12, 768
    kinds = ["bert", "llama"]
    style = {"bert": dict(ffn=3072),
             "llama": dict(ffn=2048, normalization="rms", normPlacement="pre", ffnActivation="swiglu")}
    nets = {k: TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=E, layers=12, heads=H,
                                         dataType=DataType.BFLOAT16, positionEncoding="rotary",
                                         **style[k]).init(device=DEV) for k in kinds}
    say(f"== generate() with Llama-style blocks (rms / pre / swiglu, ffnSize 2048) against post-LayerNorm GELU blocks "
        f"(ffnSize 3072) on TextGenerationTransformer(768, 12 layers, 12 heads, rotary), bf16, V = {V}, greedy, {n} new "
        f"tokens; whole calls (prompt included) on the host clock, ended by a device synchronise; median of {passes} "
        "passes (min .. max), the variants alternating within a pass; x = tokens/s against the post-LayerNorm model's "
        "same mode")
    _compare_models(nets, kinds, V, batches, n, passes)


def window_mode(window, batches, n, passes):
    """--window W: sliding-window attention in every block against none on the 12-layer, hidden-768 rotary model:
    generate() eager and graph-replayed at prefix 1024 and 4032, and a causal-LM training step at 2048 tokens."""
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, H, E = 77, 12, 768
    kinds = ["full", "window"]
    nets = {k: TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=E, layers=12, heads=H,
                                         dataType=DataType.BFLOAT16, positionEncoding="rotary",
                                         attentionWindow=window if k == "window" else None).init(device=DEV)
            for k in kinds}
    say(f"== generate() with attentionWindow = {window} in every block against no window on "
        f"TextGenerationTransformer(768, 12 layers, 12 heads, rotary), bf16, V = {V}, greedy, {n} new tokens; whole "
        f"calls (prompt included) on the host clock, ended by a device synchronise; median of {passes} passes "
        "(min .. max), the variants alternating within a pass; x = tokens/s against the model without a window, same "
        "mode")
    _compare_models(nets, kinds, V, batches, n, passes, prefixes=(1024, 4032), train=(32, 2048, 3))


def _compare_models(nets, kinds, V, batches, n, passes, prefixes=(128, 1024), train=(32, 128, 10)):
    """generate() eager and graph-replayed at the ``prefixes``, then a training step of ``train`` = (batch, tokens,
    steps per timing), of the models ``nets`` (by kind, the first the base line), the variants alternating within a
    pass."""
    say("   parameters: " + ", ".join(f"{k} {nets[k].numParams()}" for k in kinds))
    for mb in batches:
        for P in prefixes:
            prompt = torch.randint(0, V, (mb, P), generator=torch.Generator().manual_seed(mb + P)).to(DEV)
            variants = [(f"{k:7s} {mode}", nets[k], kw)
                        for mode, kw in (("eager", {}), ("graph", dict(useGraph=True))) for k in kinds]

            def call(net, kw, tokens=n):
                net.rnnClearPreviousState()
                return net.generate(prompt, maxNewTokens=tokens, **kw)

            for _, net, kw in variants:
                call(net, kw)
            times = [[] for _ in variants]
            for _ in range(passes):
                for i, (_, net, kw) in enumerate(variants):
                    times[i].append(_sync_time(lambda: call(net, kw)))
            med = [sorted(t)[len(t) // 2] for t in times]
            few = max(2, n // 4)
            short = []
            for _, net, kw in variants:
                call(net, kw, few)
                short.append(sorted(_sync_time(lambda: call(net, kw, few)) for _ in range(passes))[passes // 2])
            per = [(m - ts) / (n - few) * 1e3 for ts, m in zip(short, med)]
            for i, ((vn, _, _), t, m) in enumerate(zip(variants, times, med)):
                b = (i // len(kinds)) * len(kinds)               # the base model's row of the same mode
                say(f"batch {mb:2d} prefix {P:4d} {vn}: {mb * n / m:9.1f} tok/s  {m * 1e3:8.1f} ms per call "
                    f"({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f})  x {med[b] / m:5.3f} | step alone {per[i]:6.2f} ms  x "
                    f"{per[b] / per[i]:5.3f}")
    for net in nets.values():
        net.rnnClearPreviousState()
    say()
    B, T, steps = train
    say(f"== one causal-LM training step (fit) of the same models, batch {B}, {T} tokens, bf16: ms per step on the host "
        f"clock over {steps} steps ended by a device synchronise; median of {passes} passes (min .. max), alternating")
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, V, (B, T), generator=g).to(DEV)
    y = torch.zeros(B, V, T, device=DEV)
    y.scatter_(1, torch.randint(0, V, (B, 1, T), generator=g).to(DEV), 1.0)

    def fit(net):
        for _ in range(steps):
            net.fit([x], [y])

    for k in kinds:
        fit(nets[k])
    tt = {k: [] for k in kinds}
    for _ in range(passes):
        for k in kinds:
            tt[k].append(_sync_time(lambda: fit(nets[k])) / steps * 1e3)
    base = sorted(tt[kinds[0]])[passes // 2]
    for k in kinds:
        t = sorted(tt[k])
        say(f"{k:7s}: {t[len(t) // 2]:7.2f} ms per step ({t[0]:.2f} .. {t[-1]:.2f})  x {base / t[len(t) // 2]:5.3f}")
    say()


def speculative_kernels_mode(passes, reps):
    """The verify, commit and draft kernels of csrc/speculative.hip alone."""
    say(f"== speculative decoding kernels, bf16 distributions, K = 4, GPU time per call in us (median of {passes} "
        f"passes of {reps} launches; min .. max); verify: q == p, so every draft is accepted and all K + 1 rows are "
        "read (the most a call reads); reject@0: the first draft has p = 0, one row is read and resampled")
    K, N = 4, 16
    for mb in (1, 32):
        for V in (77, 32000, 128000):
            g = torch.Generator().manual_seed(mb + V)
            p = torch.softmax(torch.randn(K + 1, mb, V, generator=g) * 2.0, 2).to(torch.bfloat16).to(DEV)
            q = p[:K].clone()
            d = torch.multinomial(p[:K].float().reshape(K * mb, V), 1).reshape(K, mb).t().contiguous()
            p0 = p.clone()
            p0[0].scatter_(1, d[:, :1], 0.0)
            st = [torch.zeros(mb, dtype=torch.int32, device=DEV) for _ in range(3)]
            fin = torch.zeros(mb, dtype=torch.uint8, device=DEV)
            toks = torch.zeros(mb, N, dtype=torch.int64, device=DEV)
            logps = torch.zeros(mb, N, dtype=torch.float32, device=DEV)
            nxt = torch.zeros(mb, dtype=torch.int64, device=DEV)
            slot = torch.zeros(2, dtype=torch.int32, device=DEV)
            rng = PhiloxStream(DEV)

            def verify(pp, greedy):
                st[1].zero_()
                return GN.spec_verify_native(pp.permute(1, 0, 2), q.permute(1, 0, 2), d, 0.8, greedy, rng, st[0],
                                             st[1], fin, None, 0, toks, logps, nxt)

            hist = torch.randint(0, V, (mb, 193), generator=g).to(DEV)
            hlen = torch.full((mb,), 192, dtype=torch.int32, device=DEV)
            dr = torch.zeros(mb, K, dtype=torch.int64, device=DEV)
            rows = (("verify sampled", lambda: verify(p, False)), ("reject@0 sampled", lambda: verify(p0, False)),
                    ("commit", lambda: GN.spec_commit(st[0], fin, st[2], slot)),
                    ("n-gram draft, 192 tokens", lambda: GN.ngram_draft_native(hist, hlen, 3, K, dr)))
            for name, fn in rows:
                if name.startswith(("commit", "n-gram")) and V != 77:
                    continue                                     # these do not read the distributions
                t = _med(fn, passes, reps)                       # includes the zero_() launch of the cursor reset
                say(f"mb={mb:2d} V={V:6d} {name:26s}: {t[0]:8.1f} ({t[1]:.1f} .. {t[2]:.1f})")
    say()


def speculative_mode(Ks, batches, n, passes, draft_layers, lookup):
    """generate(numDraftTokens=K) against generate() on the 12-layer, hidden-768 model, alternating within a pass."""
    from deeplearning4j_amd.models import TextGenerationTransformer
    from deeplearning4j_amd.nn.conf import DataType
    V, P = 77, 128

    def model(layers, seed):
        return TextGenerationTransformer(numLabels=V, inputShape=[128], hidden=768, layers=layers, heads=12, seed=seed,
                                         maxPositions=512, dataType=DataType.BFLOAT16).init(device=DEV)
    net = model(12, 12345)
    assistant = None if lookup else model(draft_layers, 777)
    source = "prompt lookup (draftNgram 3)" if lookup else f"a {draft_layers}-layer assistant of the same width"
    say(f"== generate(numDraftTokens=K) with {source} against generate() on TextGenerationTransformer(768, 12 layers, "
        f"12 heads), bf16, V = {V}, greedy, prefix {P}, {n} new tokens; whole calls (prompt included) on the host clock, "
        f"ended by a device synchronise; median of {passes} passes (min .. max), the variants alternating within a pass")
    say("   the weights are random: the acceptance observed here says nothing about trained models. ms/round and "
        f"ms/step come from the same calls with {max(2, n // 4)} tokens (a call's time is a + b * rounds); break-even = "
        "the share of the K drafts a round must have accepted to emit tokens as fast as plain steps, "
        "(round / step - 1) / K")
    few = max(2, n // 4)
    for mb in batches:
        prompt = torch.randint(0, V, (mb, P), generator=torch.Generator().manual_seed(mb)).to(DEV)
        variants = [("plain", {})] + [(f"K={k}", dict(numDraftTokens=k, assistant=assistant)) for k in Ks]

        def call(kw, tokens):
            r = net.generate(prompt, maxNewTokens=tokens, **kw)
            return r, net.lastGenerationStats

        info = []
        for _, kw in variants:
            call(kw, few)
            info.append((call(kw, n)[1], call(kw, few)[1]))
        times = [[[], []] for _ in variants]
        for _ in range(passes):
            for i, (_, kw) in enumerate(variants):
                times[i][0].append(_sync_time(lambda: call(kw, n)))
                times[i][1].append(_sync_time(lambda: call(kw, few)))
        med = [[sorted(t)[len(t) // 2] for t in pair] for pair in times]
        step = (med[0][0] - med[0][1]) / (n - few) * 1e3
        for i, ((vn, _), (sn, sf)) in enumerate(zip(variants, info)):
            t = times[i][0]
            line = f"batch {mb:2d} {vn:6s}: {mb * n / med[i][0]:9.1f} tok/s  {med[i][0] * 1e3:8.1f} ms per call " \
                   f"({min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f})"
            if i == 0:
                line += f"  {step:6.2f} ms/step"
            else:
                rounds = max(1, sn["rounds"] - sf["rounds"])
                rnd = (med[i][0] - med[i][1]) / rounds * 1e3
                k = Ks[i - 1]
                line += f"  x {med[0][0] / med[i][0]:5.3f} | {rnd:6.2f} ms/round ({sn['rounds']} rounds), round/step " \
                        f"{rnd / step:5.2f}, break-even acceptance {(rnd / step - 1) / k:5.2f}; observed " \
                        f"{sn['acceptedTokens']}/{sn['draftTokens']} drafts accepted"
            say(line)
    net.rnnClearPreviousState()
    say()


def main():
    global _out
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sampler", action="store_true")
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--cache", choices=["fp8"], default=None,
                    help="compare generate() with the fp8 key/value cache and with the 16-bit one")
    ap.add_argument("--kv-heads", default=None,
                    help="grouped-query attention: nKVHeads values (divisors of 12, comma separated) against 12")
    ap.add_argument("--rotary", action="store_true",
                    help="rotary embeddings against learned positions: generate(), generate(useGraph=True), training")
    ap.add_argument("--positions", choices=["both", "learned", "rotary"], default="both",
                    help="--rotary: the models to measure")
    ap.add_argument("--block", choices=["llama"], default=None,
                    help="Llama-style blocks against post-LayerNorm GELU blocks: generate(), useGraph=True, training")
    ap.add_argument("--window", type=int, default=None,
                    help="sliding-window attention (attentionWindow in every block) against none: generate(), "
                         "useGraph=True at prefix 1024 and 4032, a training step at 2048 tokens")
    ap.add_argument("--speculative", default=None,
                    help="speculative decoding: numDraftTokens values (comma separated) against plain generate(), and "
                         "the verify / commit / draft kernels alone")
    ap.add_argument("--draft-layers", type=int, default=2, help="--speculative: the assistant's number of blocks")
    ap.add_argument("--lookup", action="store_true", help="--speculative: draft by prompt lookup, without an assistant")
    ap.add_argument("--tree", default=None, help="import the package from this checkout instead of the tool's own")
    ap.add_argument("--parent-lib", default=None,
                    help="kernel library built from the parent commit (--ragged, --graph)")
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
    if a.ragged:
        ragged_kernel_mode(a.passes, max(a.reps, 50), a.parent_lib)
        ragged_model_mode(a.tokens, a.passes)
    if a.graph:
        graph_mode(a.batch, a.tokens, a.passes, a.parent_lib)
    if a.cache:
        cache_fp8_mode(a.batch, a.tokens, a.passes)
    if a.kv_heads:
        kv_heads_mode([int(h) for h in a.kv_heads.split(",")], a.batch, a.tokens, a.passes)
    if a.rotary:
        rotary_mode(a.batch, a.tokens, a.passes, a.positions)
    if a.block:
        block_mode(a.batch, a.tokens, a.passes)
    if a.window:
        window_mode(a.window, a.batch, a.tokens, a.passes)
    if a.speculative:
        speculative_kernels_mode(a.passes, a.reps)
        speculative_mode([int(k) for k in a.speculative.split(",")], a.batch, a.tokens, a.passes, a.draft_layers,
                         a.lookup)


if __name__ == "__main__":
    main()
