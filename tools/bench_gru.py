#!/usr/bin/env python3
"""GRU / SimpleRnn counterpart of tools/bench_lstm.py: the char-LM configuration (2 recurrent layers of 256 units ->
RnnOutputLayer, RmsProp(0.01), l2 1e-3, truncated BPTT 50/50, 77 characters, minibatch 32, 1000-character sequences)
with GRU or SimpleRnn layers, in characters/sec. Passes alternate between the whole-sequence kernels (csrc/gru.hip)
and the per-step path (DL4J_AMD_KERNEL_GRU=0 / DL4J_AMD_KERNEL_RNN=0, which for SimpleRnn is the code every
SimpleRnn ran before the kernels existed) inside one process, so both see the same clocks; one JSON line gives every
pass and the spread between passes.

Usage: python tools/bench_gru.py --cell gru|rnn [--passes P --steps K --warmup W --dtype bf16|fp32]
       python tools/bench_gru.py --kernels     per-step time of the GRU / RNN sequence kernels against the
                                               single-workgroup LSTM kernel at the same H and mb
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _net(cell, args, dev):
    from deeplearning4j_amd import (Activation, BackpropType, DataType, GRU, InputType, LossFunction,
                                    MultiLayerNetwork, NeuralNetConfiguration, RmsProp, RnnOutputLayer, SimpleRnn,
                                    WeightInit)
    L = GRU if cell == "gru" else SimpleRnn
    dt = DataType.BFLOAT16 if args.dtype == "bf16" else DataType.FLOAT
    conf = (NeuralNetConfiguration.Builder().seed(12345).dataType(dt).l2(0.001).weightInit(WeightInit.XAVIER)
            .updater(RmsProp(0.01)).list()
            .layer(0, L.Builder().nIn(args.chars).nOut(args.hidden).activation(Activation.TANH).build())
            .layer(1, L.Builder().nOut(args.hidden).activation(Activation.TANH).build())
            .layer(2, RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nOut(args.chars).build())
            .setInputType(InputType.recurrent(args.chars))
            .backpropType(BackpropType.TruncatedBPTT).tBPTTForwardLength(50).tBPTTBackwardLength(50).build())
    net = MultiLayerNetwork(conf)
    net.init(device=dev)
    return net


def _time(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench_cell(args, dev):
    env = "DL4J_AMD_KERNEL_" + ("GRU" if args.cell == "gru" else "RNN")
    g = torch.Generator().manual_seed(7)
    idx = torch.randint(0, args.chars, (args.batch, args.length + 1), generator=g)
    x = torch.nn.functional.one_hot(idx[:, :-1], args.chars).permute(0, 2, 1).float().to(dev)
    y = torch.nn.functional.one_hot(idx[:, 1:], args.chars).permute(0, 2, 1).float().to(dev)
    nets = {m: _net(args.cell, args, dev) for m in ("kernels", "per_step")}
    res = {m: [] for m in nets}
    for p in range(args.passes + 1):                           # pass 0 warms both modes up and is not reported
        for mode, net in nets.items():
            os.environ[env] = "1" if mode == "kernels" else "0"
            for _ in range(args.warmup):
                net.fit(x, y)
            s = _time(lambda: net.fit(x, y), args.steps)
            if p:
                res[mode].append(round(args.batch * args.length / s, 1))
    os.environ[env] = "1"
    mean = {m: sum(v) / len(v) for m, v in res.items()}
    print(json.dumps({"metric": f"characters/sec 2x {args.cell.upper()}-{args.hidden} char-LM training (TBPTT 50)",
                      "unit": "chars/sec", "dtype": args.dtype, "passes": res,
                      "mean": {m: round(v, 1) for m, v in mean.items()},
                      "spread_pct": {m: round(100 * (max(v) - min(v)) / mean[m], 2) for m, v in res.items()},
                      "speedup": round(mean["kernels"] / mean["per_step"], 2)}), flush=True)


def bench_kernels(args, dev):
    from deeplearning4j_amd.ops import rnn_native as RN
    os.environ["DL4J_AMD_LSTM_COOP"] = "0"                     # the single-workgroup LSTM kernel
    H, mb, T = args.hidden, args.batch, 50
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    eps, out = rnd(T, mb, H), {}
    for name, G in (("lstm", 4), ("gru", 3), ("rnn", 1)):
        zx, RW = (rnd(T, mb, G * H) * 0.5).to(dt), (rnd(H, G * H) / H ** 0.5).to(dt)
        if name == "lstm":
            packs = RN.pack_rw(RW, H, False)
            fwd = lambda: RN.lstm_seq_fwd(zx, RW, H, False, packs=packs)  # noqa: E731
            o, _, _, gates, call, _ = fwd()
            bwd = lambda: RN.lstm_seq_bwd(eps, gates, call, None, RW, H, False, packs=packs)  # noqa: E731
        elif name == "gru":
            packs = RN.pack_rw_blocks(RW, H, 3)
            fwd = lambda: RN.gru_seq_fwd(zx, RW, torch.zeros(H, device=dev), H, packs=packs)  # noqa: E731
            o, _, gates, _ = fwd()
            bwd = lambda: RN.gru_seq_bwd(eps, gates, o, None, RW, H, packs=packs)  # noqa: E731
        else:
            packs = RN.pack_rw_blocks(RW, H, 1)
            fwd = lambda: RN.rnn_seq_fwd(zx, RW, H, "tanh", packs=packs)  # noqa: E731
            o = fwd()[0]
            bwd = lambda: RN.rnn_seq_bwd(eps, o, RW, H, "tanh", packs=packs)  # noqa: E731
        for f in (fwd, bwd):
            _time(f, 5)
        out[name] = {"fwd_us_per_step": [round(_time(fwd, 50) / T * 1e6, 3) for _ in range(args.passes)],
                     "bwd_us_per_step": [round(_time(bwd, 50) / T * 1e6, 3) for _ in range(args.passes)]}
    print(json.dumps({"metric": "sequence kernel time per time step (launch included, T = 50)", "H": H, "mb": mb,
                      "dtype": args.dtype, "kernels": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", default="gru", choices=["gru", "rnn"])
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--chars", type=int, default=77)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    (bench_kernels if args.kernels else bench_cell)(args, dev)


if __name__ == "__main__":
    main()
