"""SHA-256 digests of kernel outputs from one build of the kernel library, to compare two builds bit for bit.

    python tools/output_digests.py LIBDIR OUT.txt      # one process per library: run it once for each build
    python tools/output_digests.py --compare A.txt B.txt

LIBDIR holds ``libdl4j_amd_kernels.so`` (this tree's is ``deeplearning4j_amd/_lib``); the Python side is always this
tree's, so a library built from another commit must still export what this tree's header declares. The run is
deterministic (DL4J_AMD_DETERMINISTIC=1) with the conv and GEMM tuners off, so both builds launch the same kernel for
every call: with a tuner on, two processes can time their way to different tiles and differ legitimately.

Covered, at the shapes of the GPU tests: the conv layer path (y, dx with and without accumulation, dW, db; the 1x1
cases are the backward-data GEMM), every tile-engine variant forward with tile statistics, backward-data with and
without accumulation and weight gradient, GEMMs with forward tile statistics on every tile configuration, BatchNorm
forward / backward plain, ReLU, residual with mask, residual with the shortcut BN folded in (RBN) and fed by conv tile
statistics at every fold path, and the fused BN + pool forward / backward.
"""
import hashlib
import os
import sys

os.environ["DL4J_AMD_DETERMINISTIC"] = "1"
os.environ["DL4J_AMD_CONV_TUNE"] = "0"
os.environ["DL4J_AMD_GEMM_TUNE"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONV_CASES = [   # tests/test_gpu_conv.py: N, C, H, W, K, R, S, stride, pad4 (t, b, l, r)
    (2, 64, 9, 9, 64, 1, 1, (1, 1), (0, 0, 0, 0)),
    (3, 64, 8, 7, 256, 1, 1, (1, 1), (0, 0, 0, 0)),
    (2, 128, 11, 11, 64, 1, 1, (2, 2), (0, 0, 0, 0)),
    (2, 64, 10, 9, 64, 3, 3, (1, 1), (1, 1, 1, 1)),
    (2, 32, 7, 7, 136, 3, 3, (1, 1), (0, 1, 0, 1)),
    (2, 8, 23, 23, 64, 7, 7, (2, 2), (3, 3, 3, 3)),
    (1, 256, 5, 5, 512, 3, 3, (1, 1), (1, 1, 1, 1)),
    (4, 512, 4, 4, 2048, 1, 1, (1, 1), (0, 0, 0, 0)),
    (2, 48, 6, 6, 64, 3, 3, (1, 1), (1, 1, 1, 1)),
    (3, 96, 9, 9, 64, 3, 3, (2, 2), (1, 1, 1, 1)),
]
V3_CASES = [     # tests/test_gpu_conv_v3.py: ..., dilation; CASES are the first seven, WRW_CASES those in V3_WRW
    (2, 64, 9, 9, 64, 3, 3, (1, 1), (1, 1, 1, 1), (1, 1)),
    (3, 128, 7, 7, 136, 3, 3, (1, 1), (1, 1, 1, 1), (1, 1)),
    (2, 64, 11, 13, 256, 1, 1, (1, 1), (0, 0, 0, 0), (1, 1)),
    (2, 192, 10, 10, 72, 3, 3, (2, 2), (1, 1, 1, 1), (1, 1)),
    (1, 64, 12, 12, 64, 3, 3, (1, 1), (2, 2, 2, 2), (2, 2)),
    (2, 64, 8, 8, 512, 5, 5, (1, 1), (2, 2, 2, 2), (1, 1)),
    (5, 128, 6, 5, 128, 3, 3, (1, 1), (0, 1, 0, 1), (1, 1)),
    (4, 256, 8, 8, 64, 1, 1, (2, 2), (0, 0, 0, 0), (1, 1)),
    (2, 8, 23, 23, 64, 7, 7, (2, 2), (3, 3, 3, 3), (1, 1)),
]
V3_WRW = (0, 1, 2, 3, 4, 7, 8)
BN_SHAPES = [(4, 64, 9, 7), (2, 256, 5, 5), (3, 2048, 2, 2), (16, 24), (200, 64, 32, 32), (500000, 24),
             (64, 256, 16, 16)]                                    # tests/test_gpu_kernels.py
BN_RES_SHAPES = [(4, 64, 6, 5), (200, 64, 32, 32)]
BN_TILE_FED = [(2, 20), (16, 50), (8, 256), (9, 256)]              # P = 25 / 625 / 8192 / 9216 tile partials
BNPOOL_CASES = [((4, 64, 28, 28), 3, 2, (1, 1, 1, 1)), ((3, 16, 13, 11), 3, 2, (0, 0, 0, 0)),
                ((2, 8, 10, 10), 2, 2, (0, 0, 0, 0))]              # tests/test_gpu_bnpool.py
GEMM_STATS_CFGS = [None, (0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (8, 1), (9, 1)]   # tests/test_gpu_gemm.py


def dump(libdir, out_path):
    import torch
    from deeplearning4j_amd.ops import native
    native.KERNEL_LIB = os.path.join(os.path.abspath(libdir), "libdl4j_amd_kernels.so")
    from deeplearning4j_amd.ops import conv_native, gemm
    lib = native.load()
    dev = torch.device("cuda", 0)
    lines = []

    def put(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            if t is None:
                continue
            raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
            lines.append(f"{name}[{i}] {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}")

    def cl(t):
        return t.to(dev).contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.to(dev)

    def out_hw(H, W, R, S, stride, pad4, dil=(1, 1)):
        return ((H + pad4[0] + pad4[1] - dil[0] * (R - 1) - 1) // stride[0] + 1,
                (W + pad4[2] + pad4[3] - dil[1] * (S - 1) - 1) // stride[1] + 1)

    # ---- conv layer path (its 1x1 cases run forward and backward data as GEMMs)
    for dt in (torch.bfloat16,):
        for ci, (N, C, H, W, K, R, S, stride, pad4) in enumerate(CONV_CASES):
            g = torch.Generator().manual_seed(5)
            x = cl(torch.randn(N, C, H, W, generator=g).to(dt))
            w = (torch.randn(K, C, R, S, generator=g) * 0.1).to(dev).to(dt)
            b = torch.randn(K, generator=g).to(dev).to(dt)
            OH, OW = out_hw(H, W, R, S, stride, pad4)
            dy = cl(torch.randn(N, K, OH, OW, generator=g).to(dt))
            other = cl(torch.randn(N, C, H, W, generator=g).to(dt))
            conv_native.bump_version()
            tag = f"conv_layer {str(dt)[6:]} case{ci}"
            for stats in (False, True):
                y = conv_native.conv2d_fwd(x, w, b, stride, pad4, (1, 1), want_stats=stats)
                if y is not None:
                    put(f"{tag} fwd stats={int(stats)}", y)
            r = conv_native.conv2d_bwd(x, w, dy, stride, pad4, (1, 1), True, True, True)
            if r is not None:
                put(f"{tag} bwd", *r)
            r = conv_native.conv2d_bwd(x, w, dy, stride, pad4, (1, 1), True, False, False, dx_accum=other.clone())
            if r is not None:
                put(f"{tag} bwd_acc", r[0])

    # ---- every tile-engine variant, directly
    nv, nvw = lib.dl4j_conv_v3_num_variants(), lib.dl4j_conv_wrw_v3_num_variants()
    for ci, (N, C, H, W, K, R, S, stride, pad4, dil) in enumerate(V3_CASES):
        g = torch.Generator().manual_seed(3)
        x = cl(torch.randn(N, C, H, W, generator=g).bfloat16())
        w = (torch.randn(K, C, R, S, generator=g) * 0.1).to(dev).bfloat16()
        b = torch.randn(K, generator=g).to(dev)
        OH, OW = out_hw(H, W, R, S, stride, pad4, dil)
        dy = cl(torch.randn(N, K, OH, OW, generator=g).bfloat16())
        base = cl(torch.randn(N, C, H, W, generator=g).bfloat16())
        geom = (N, H, W, C, K, R, S, stride[0], stride[1], pad4[0], pad4[2], dil[0], dil[1], OH, OW)
        conv_native.bump_version()
        if ci < 7 and conv_native._v3_ok(C, K, R, S):
            krsc, _ = conv_native._relayout(w, True, False)
            for v in range(nv):
                y = torch.zeros_like(dy)
                ts = conv_native._stats_buf(v, N * OH * OW, K, dev, geom).zero_()
                if conv_native._fwd_launch(v, x, krsc, b, y, geom, 0.0, ts) == 1:
                    put(f"v3 case{ci} fwd var{v}", y, ts)
        if ci < 7 and stride == (1, 1) and dil == (1, 1) and conv_native._v3_ok(K, C, R, S):
            _, flip = conv_native._relayout(w, False, True)
            gb = (N, OH, OW, K, C, R, S, 1, 1, R - 1 - pad4[0], S - 1 - pad4[2], 1, 1, H, W)
            for v in range(nv):
                for acc in (False, True):
                    dx = base.clone() if acc else torch.zeros_like(base)
                    if conv_native._fwd_launch(v, dy, flip, None, dx, gb, 1.0 if acc else 0.0, None) == 0:
                        put(f"v3 case{ci} bwd_data var{v} acc={int(acc)}", dx)
        for v in range(nvw) if ci in V3_WRW else ():
            dW = torch.zeros((K, C, R, S), device=dev)
            db = torch.zeros((K,), device=dev)
            if conv_native._wrw_v3_launch(v, x, dy, dW, geom, db if v % 2 else None) == 0:
                put(f"v3 case{ci} wrw var{v}", dW, db if v % 2 else None)

    # ---- GEMM with forward tile statistics, every tile configuration
    for dt in (torch.bfloat16,):
        for M, N, K in ((1000, 192, 128), (1024, 256, 64)):
            g = torch.Generator().manual_seed(10)
            a = torch.randn(M, K, generator=g).to(dev).to(dt)
            b = torch.randn(N, K, generator=g).to(dev).to(dt).t()
            bias = torch.randn(N, generator=g).to(dev)
            for cfg in GEMM_STATS_CFGS + [(10, 1)]:
                ts = torch.zeros((3, 2 * ((M + 127) // 128), N), device=dev)
                gemm._FORCE_CFG = cfg
                try:
                    out = gemm.mmul(a, b, bias=bias, stats=ts)
                except RuntimeError as e:                       # a configuration that refuses the shape
                    lines.append(f"gemm_stats {str(dt)[6:]} {M}x{N}x{K} cfg={cfg} refused: {e}")
                    continue
                finally:
                    gemm._FORCE_CFG = None
                put(f"gemm_stats {str(dt)[6:]} {M}x{N}x{K} cfg={cfg}", out, ts)

    # ---- BatchNorm
    def bn_params(C, g):
        return ((torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev),
                torch.zeros(C, device=dev), torch.ones(C, device=dev))

    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for shape in BN_SHAPES:
            for relu in (False, True):
                g = torch.Generator().manual_seed(0)
                x = cl((torch.randn(*shape, generator=g) * 3 + 1.5).to(dt))
                gamma, beta, rm, rv = bn_params(shape[1], g)
                dy = cl(torch.randn(*shape, generator=g).to(dt))
                r = native.bn_fwd(x, gamma, beta, rm, rv, True, 0.9, 1e-5, relu)
                if r is None:
                    continue
                tag = f"bn {str(dt)[6:]} {shape} relu={int(relu)}"
                put(tag + " fwd", r[0], r[1][2], rm, rv)
                put(tag + " bwd", *native.bn_bwd(dy, r[1]))
        for shape in BN_RES_SHAPES:
            g = torch.Generator().manual_seed(7)
            x = cl((torch.randn(*shape, generator=g) * 2 + 0.5).to(dt))
            res = cl(torch.randn(*shape, generator=g).to(dt))
            dy = cl(torch.randn(*shape, generator=g).to(dt))
            gamma, beta, rm, rv = bn_params(shape[1], g)
            r = native.bn_fwd(x, gamma, beta, rm, rv, True, 0.9, 1e-5, True, residual=res)
            if r is not None:
                put(f"bn_res {str(dt)[6:]} {shape} fwd", r[0], r[1][2], r[1][7], rm, rv)
                put(f"bn_res {str(dt)[6:]} {shape} bwd", *native.bn_bwd(dy, r[1]))
            if dt == torch.float32:
                continue                                         # RBN: 16-bit only
            g2, b2, rm2, rv2 = bn_params(shape[1], g)
            sc = native.bn_fwd(res, g2, b2, rm2, rv2, True, 0.9, 1e-5, False, stats_only=True)
            r = native.bn_fwd(x, gamma, beta, rm, rv, True, 0.9, 1e-5, True, residual=res, rctx=sc[1][2])
            put(f"bn_rbn {str(dt)[6:]} {shape} fwd", r[0], r[1][2], r[1][7], sc[1][2], rm, rv, rm2, rv2)
            dg2, db2 = torch.zeros(shape[1], device=dev), torch.zeros(shape[1], device=dev)
            put(f"bn_rbn {str(dt)[6:]} {shape} bwd", *native.bn_bwd(dy, r[1], rgrads=(dg2, db2)), dg2, db2)

    # ---- BN (plain, residual, RBN) and BN + pool fed by the producing conv's tile statistics, every fold path
    for N, H in BN_TILE_FED:
        C = 64
        g = torch.Generator().manual_seed(4)
        x = cl((torch.randn(N, C, H, H, generator=g) + 0.2).bfloat16())
        w = (torch.randn(C, C, 3, 3, generator=g) * 0.05).to(dev).bfloat16()
        gamma, beta, rm, rv = bn_params(C, g)
        conv_native.bump_version()
        y = conv_native.conv2d_fwd(x, w, None, (1, 1), (1, 1, 1, 1), (1, 1), want_stats=True)
        assert hasattr(y, "_bn_tile_stats"), "the conv produced no tile statistics"
        r = native.bn_fwd(y, gamma, beta, rm, rv, True, 0.9, 1e-5, True)
        put(f"bn_tiles N={N} H={H} fwd", r[0], r[1][2], rm, rv)
        put(f"bn_tiles N={N} H={H} bwd", *native.bn_bwd(x, r[1]))
        r = native.bn_fwd(y, gamma, beta, rm, rv, True, 0.9, 1e-5, True, residual=x)
        put(f"bn_tiles_res N={N} H={H} fwd", r[0], r[1][2], r[1][7], rm, rv)
        sc = native.bn_fwd(x, gamma, beta, rm.clone(), rv.clone(), True, 0.9, 1e-5, False, stats_only=True)
        r = native.bn_fwd(y, gamma, beta, rm, rv, True, 0.9, 1e-5, True, residual=x, rctx=sc[1][2])
        put(f"bn_tiles_rbn N={N} H={H} fwd", r[0], r[1][2], r[1][7], rm, rv)
        if N * H * H <= 1 << 20:
            rp = native.bn_pool_fwd(y, gamma, beta, rm, rv, True, 0.9, 1e-5, (3, 3), (2, 2), (1, 1, 1, 1))
            if rp is not None:
                put(f"bnpool_tiles N={N} H={H} fwd", rp[0], rp[1][2], rp[1][3], rp[1][4], rm, rv)

    for dt in (torch.float32, torch.bfloat16):
        for shape, k, s, pad in BNPOOL_CASES:
            g = torch.Generator().manual_seed(shape[1] + k)
            x = cl((torch.randn(shape, generator=g) * 1.5 + 0.3).to(dt))
            gamma, beta, rm, rv = bn_params(shape[1], g)
            rp = native.bn_pool_fwd(x, gamma, beta, rm, rv, True, 0.9, 1e-5, (k, k), (s, s), pad)
            if rp is None:
                continue
            tag = f"bnpool {str(dt)[6:]} {shape} k={k}"
            put(tag + " fwd", rp[0], rp[1][2], rp[1][3], rp[1][4], rm, rv)
            dy = cl(torch.randn(rp[0].shape, generator=g).to(dt))
            put(tag + " bwd", *native.bn_pool_bwd(dy, rp[1]))

    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} digests from {native.KERNEL_LIB} -> {out_path}")


def compare(pa, pb):
    a, b = open(pa).read().splitlines(), open(pb).read().splitlines()
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in diff:
        print(f"- {x}\n+ {y}")
    print(f"{len(a)} / {len(b)} digests, {len(diff)} differ" + ("" if len(a) == len(b) else " (counts differ)"))
    return 0 if not diff and len(a) == len(b) else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    dump(sys.argv[1], sys.argv[2])
