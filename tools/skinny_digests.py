"""SHA-256 digests of the outputs of the four decode products (dl4j_skinny_gemm, dl4j_skinny_gemm_grouped, dl4j_wq_gemm,
dl4j_wq_gemm_grouped) from one build of the kernel library, to compare two builds bit for bit.

    python tools/skinny_digests.py LIBDIR OUT.txt      # one process per library: run it once for each build
    python tools/output_digests.py --compare A.txt B.txt

LIBDIR holds ``libdl4j_amd_kernels.so`` (this tree's is ``deeplearning4j_amd/_lib``); the Python side is always this
tree's. Operands: the exact ones of tests/_exact_operands.py and random ones.

Dense, both families: M in {1, 3, 17, 64} x beta 0 / 1 x GELU on / off x bias fp32 / 16-bit x aligned / unaligned out,
bf16 and fp16. 16-bit: (K, N) in {(8, 8), (40, 24), (96, 77), (768, 256)} and the split (3, 3072, 80), K-contiguous
and both load widths. Quantised: (K, N) in {(32, 16), (96, 77), (288, 40), (544, 33)} (the last two split), fp8 and
fp4. Grouped, both families: Ntok in {1, 17, 64} x gather / sorted x both planted plans (each has idle experts) x GELU
on / off x aligned / unaligned out, at an unsplit shape and one that splits K."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MS = (1, 3, 17, 64)
SKINNY_KN = ((8, 8), (40, 24), (96, 77), (768, 256))
SKINNY_SPLIT = (3, 3072, 80)
WQ_KN = ((32, 16), (96, 77), (288, 40), (544, 33))
NTOK = (1, 17, 64)
SKINNY_GROUPED_KN = ((40, 24), (520, 136))
WQ_GROUPED_KN = ((96, 77), (544, 33))
NAN = float("nan")


def dump(libdir, out_path):
    import torch
    import _exact_operands as EO
    from deeplearning4j_amd.ops import native
    native.KERNEL_LIB = os.path.join(os.path.abspath(libdir), "libdl4j_amd_kernels.so")
    from deeplearning4j_amd.ops import fallback
    from deeplearning4j_amd.ops import transformer_native as TN
    native.load()
    fallback.reset()
    dev = torch.device("cuda", 0)
    lines = []

    def put(name, buf):
        raw = buf.contiguous().cpu().view(torch.uint8).numpy().tobytes()
        lines.append(f"{name} {tuple(buf.shape)} {hashlib.sha256(raw).hexdigest()}")

    def framed(t, dt):
        R, C = t.shape
        buf = torch.full((R, (C + 7) // 8 * 8 + 8), NAN, dtype=dt, device=dev)
        buf[:, :C] = t.to(dt).to(dev)
        return buf[:, :C]

    def frame(rows, N, dt, aligned, init):
        """(the whole buffer, its [rows, N] corner): pitch a multiple of 8, or N + 5; NaN around, ``init`` inside."""
        buf = torch.full((rows + 2, (N + 7) // 8 * 8 + 8 if aligned else N + 5), NAN, dtype=dt, device=dev)
        buf[:rows, :N] = init
        return buf, buf[:rows, :N]

    def dense_operands(kind, fmt, M, K, N):
        if kind == "exact":
            return EO.dense(M, K, N) if fmt is None else EO.mx(fmt, M, K, N)
        g = EO.gen("digest dense", fmt, M, K, N)
        return (torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.1, torch.randn(N, generator=g),
                torch.randn(M, N, generator=g))

    def dense(tag, call, x, bias, c0, dt):
        """the 16 epilogues of one product; the digest covers the NaN frame too"""
        M, N = c0.shape
        xg = framed(x, dt)
        for i in range(16):
            beta, gelu, b16, aligned = float(i & 1), bool(i & 2), bool(i & 4), bool(i & 8)
            buf, out = frame(M, N, dt, aligned, c0.to(dt).to(dev))
            r = call(xg, (bias.to(dt) if b16 else bias.float()).to(dev), "gelu" if gelu else None, out, beta)
            assert r is out and fallback.count() == 0, f"{tag}: {fallback.summary()}"
            put(f"{tag} beta={beta} gelu={int(gelu)} bias16={int(b16)} aligned={int(aligned)}", buf)

    for dt in EO.DTS:
        dn = str(dt)[6:]
        # ---- dense
        for kind in ("exact", "random"):
            for M, K, N in [(M, K, N) for K, N in SKINNY_KN for M in MS] + [SKINNY_SPLIT]:
                x, w, bias, c0 = dense_operands(kind, None, M, K, N)
                for lay, width in (("n", 4), ("n", 8), ("k", 0)):
                    wg = framed(w, dt) if lay == "n" else framed(w.t(), dt).t()
                    dense(f"skinny {kind} {dn} {lay}{width} M={M} K={K} N={N}",
                          lambda xg, bg, act, out, beta: TN.skinny_gemm(xg, wg, bg, act, out, beta, width=width),
                          x, bias, c0, dt)
            for fmt in EO.FMTS:
                for K, N in WQ_KN:
                    for M in MS:
                        x, w, bias, c0 = dense_operands(kind, fmt, M, K, N)
                        qw = TN.wq_quantize(w.to(dt).to(dev), fmt)
                        dense(f"wq {kind} {dn} {fmt} M={M} K={K} N={N}",
                              lambda xg, bg, act, out, beta: TN.wq_gemm(xg, qw, bg, act, out, beta), x, bias, c0, dt)
        # ---- grouped
        for kind in ("exact", "random"):
            for fmt, kns in ((None, SKINNY_GROUPED_KN),) + tuple((f, WQ_GROUPED_KN) for f in EO.FMTS):
                for K, N in kns:
                    for Ntok in NTOK:
                        if kind == "exact":
                            x, w, bias = EO.grouped(fmt, K, N, Ntok)
                        else:
                            g = EO.gen("digest grouped", fmt, K, N, Ntok)
                            x, w, bias = (torch.randn(Ntok, K, generator=g), torch.randn(EO.X, K, N, generator=g) * 0.1,
                                          torch.randn(EO.X, N, generator=g))
                        bg = bias.float().to(dev)
                        if fmt is None:
                            flat = framed(w.reshape(EO.X * K, N), dt)
                            wg = flat.as_strided((EO.X, K, N), (K * flat.stride(0), flat.stride(0), 1))
                            variants = [(f"width {wd}", lambda *a, wd=wd: TN.skinny_gemm_grouped(
                                a[0], wg, bg, a[1], a[2], a[3], a[4], width=wd)) for wd in (4, 8)]
                        else:
                            qe = TN.wq_quantize_experts(w.to(dt).to(dev), fmt)
                            variants = [(fmt, lambda *a: TN.wq_gemm_grouped(a[0], qe, bg, a[1], a[2], a[3], a[4]))]
                        for pk in EO.PLANS:
                            p = EO.plan(pk, Ntok)
                            a, live = EO.grouped_rows(p, x)
                            gp = p._replace(**{f: getattr(p, f).to(dev) for f in ("cnt", "off", "src_of")})
                            for gather in (True, False):
                                xin = x if gather else torch.where(live.unsqueeze(1), a, torch.full_like(a, NAN))
                                xg = framed(xin, dt)
                                for vn, call in variants:
                                    for i in range(4):
                                        gelu, aligned = bool(i & 1), bool(i & 2)
                                        buf, out = frame(p.rows, N, dt, aligned, NAN)
                                        r = call(xg, gp, gather, "gelu" if gelu else None, out)
                                        tag = (f"grouped {kind} {dn} {vn} K={K} N={N} Ntok={Ntok} plan={pk} "
                                               f"gather={int(gather)} gelu={int(gelu)} aligned={int(aligned)}")
                                        assert r is out and fallback.count() == 0, f"{tag}: {fallback.summary()}"
                                        put(tag, buf)

    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} digests from {native.KERNEL_LIB} -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    dump(sys.argv[1], sys.argv[2])
