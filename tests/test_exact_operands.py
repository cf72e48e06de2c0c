"""The operands of tests/test_gpu_gemm_exact.py, checked on the CPU: for every product that file launches, every
partial sum is an fp32 value (so "bit-equal to fp64 rounded once" is what a correct kernel must give), the MX weights
survive the reference quantiser unchanged with several distinct scale bytes, and each planted error of a kernel (a
dropped k row, two columns exchanged within an 8-row slab, a neighbouring group's scale) changes the expected bits."""
import pytest
import torch

import _exact_operands as EO
from deeplearning4j_amd.ops import transformer_native as TN


def _cases():
    return list(EO.products())


def test_every_product_is_exact_in_fp32_in_any_order():
    n = 0
    for label, x, w, extra, dts, _ in _cases():
        EO.assert_exact(x, w, extra, dts)
        ref = x @ w
        rows = slice(0, min(x.shape[0], 64))               # the rows of a product are independent
        perm = torch.randperm(x.shape[1], generator=EO.gen("perm", label))
        got = x[rows].float()[:, perm] @ w.float()[perm]
        assert torch.equal(got.double(), ref[rows]), label
        assert torch.equal(ref.float().double(), ref), label
        for dt in dts:                                     # double -> dt is float -> dt
            assert torch.equal(EO.bits(EO.expected(ref, dt)), EO.bits(ref.float().to(dt))), label
        n += 1
    assert n > 300


def test_the_reference_quantiser_is_exact_on_grid_weights():
    for label, x, w, extra, dts, fmt in _cases():
        if fmt is None:
            continue
        for dt in dts:
            qw = TN.wq_quantize_reference(w.to(dt), fmt)
            assert torch.equal(TN.wq_dequantize_reference(qw, torch.float64), w), label
        # the pad groups' byte (127) is not counted, even where a live group carries it too
        assert (qw.scales.unique() != 127).sum() >= 4, label


def test_the_format_refuses_the_depths_that_are_no_multiple_of_32():
    for K, N in EO.WQ_REFUSED_KN:
        for fmt in EO.FMTS:
            with pytest.raises(ValueError):
                TN.wq_quantize_reference(torch.zeros(K, N), fmt)


def test_planted_errors_change_the_expected_bits():
    for label, x, w, extra, dts, fmt in _cases():
        K, N = w.shape
        ref = x @ w
        last = ref - x[:, -1:] * w[-1:]                                        # the last k row dropped
        mutants = [("last k row", last)]
        if N > 1:
            slab = slice(K // 8 // 2 * 8, min(K, K // 8 // 2 * 8 + 8))
            c1, c2 = N // 3, N - 1
            swap = ref.clone()                                                 # two columns exchanged within a slab
            swap[:, c1] += x[:, slab] @ (w[slab, c2] - w[slab, c1])
            swap[:, c2] += x[:, slab] @ (w[slab, c1] - w[slab, c2])
            mutants.append(("columns exchanged in a slab", swap))
        if fmt is not None:
            grp = slice(K // 32 // 2 * 32, K // 32 // 2 * 32 + 32)
            # one k group's scales doubled (in every column: with one row, a single column's sum may round the same)
            mutants.append(("a group's scale doubled", ref + x[:, grp] @ w[grp]))
        for dt in dts:
            want = EO.bits(EO.expected(ref, dt))
            for name, bad in mutants:
                assert not torch.equal(EO.bits(EO.expected(bad, dt)), want), f"{label} {dt}: {name} goes unseen"
