"""Weight-only MXFP8 / MXFP4 decoding off the GPU: the format as the torch reference functions of
ops/transformer_native.py write it, the refusals of rnnSetWeightDataType, and an fp64 network whose rnnTimeStep reads
the quantised copies (against the same network holding the dequantised values), also after a parameter update."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import transformer_native as TN

CPU = torch.device("cpu")
FMTS = ["fp8", "fp4"]
TOP = {"fp8": 448.0, "fp4": 6.0}


def _representable(fmt, K, N, seed=0):
    """[K, N] of values code * 2^ex the format holds exactly, every group with a code of the largest magnitude (so
    the quantiser finds the same exponent again)."""
    g = torch.Generator().manual_seed(seed)
    if fmt == "fp8":
        codes = torch.randint(0, 256, (K, N), generator=g, dtype=torch.uint8)
        codes[(codes & 0x7f) == 0x7f] = 0x10                                      # no NaN codes
        v = codes.view(torch.float8_e4m3fn).float()
    else:
        c = torch.randint(0, 16, (K, N), generator=g)
        v = torch.tensor(TN._E2M1)[c & 7] * torch.where(c > 7, -1.0, 1.0)
    v[::32] = TOP[fmt]
    ex = torch.randint(-9, 4, (K // 32, N), generator=g)
    return torch.ldexp(v.reshape(K // 32, 32, N), ex.unsqueeze(1)).reshape(K, N)


@pytest.mark.parametrize("K,N", [(32, 16), (96, 77)])
@pytest.mark.parametrize("fmt", FMTS)
def test_reference_round_trips_representable_values(fmt, K, N):
    w = _representable(fmt, K, N)
    qw = TN.wq_quantize_reference(w, fmt)
    assert qw.codes.numel() * 8 == -(-K // 64) * 64 * -(-N // (128 // qw.bits)) * (128 // qw.bits) * qw.bits
    assert torch.equal(TN.wq_dequantize_reference(qw, torch.float32), w)
    for dt in (torch.bfloat16, torch.float16):                     # exact in both 16-bit types
        assert torch.equal(TN.wq_dequantize_reference(qw, dt).float(), w)


@pytest.mark.parametrize("fmt", FMTS)
def test_reference_special_groups(fmt):
    top = TOP[fmt]
    w = torch.zeros(128, 3)
    w[32:64, 0] = 0.01
    w[40, 0] = 1e30                                                # one huge element: the rest of its group vanishes
    w[64:96, 1] = torch.linspace(-1.0, 1.0, 32) * top              # the maximum exactly at 448 / 6: ex = 0
    w[96:128, 2] = top * 1.0001                                    # just above: the next exponent
    qw = TN.wq_quantize_reference(w, fmt)
    d = TN.wq_dequantize_reference(qw, torch.float32)
    sc = qw.scales.reshape(-1, 2, 16, 8 // qw.bits, 2)[0, :, :3, 0, :].permute(0, 2, 1).reshape(4, 3)   # [group, column]
    assert sc[0].tolist() == [127, 127, 127] and d[:32].abs().max() == 0        # all-zero groups: scale byte 127
    assert d[32:64, 0].abs().sum() == d[40, 0] and 0.5e30 < d[40, 0] < 1.5e30
    assert sc[2, 1] == 127 and d[64, 1] == -top and d[95, 1] == top
    assert sc[3, 2] == 128 and d[96, 2] <= top * 1.0001
    # every value is within half a code step of its group's scale (nearest rounding, no saturation loss)
    step = (2.0 ** (sc.float() - 127)).repeat_interleave(32, 0) * (32.0 if fmt == "fp8" else 1.0)
    assert ((d - w).abs() <= step)[64:].all()


def _lm(fmt=None, dtype=DataType.DOUBLE, llama=False, hidden=64, seed=7):
    kw = dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu", positionEncoding="rotary") if llama \
        else {}
    return TextGenerationTransformer(numLabels=77, seed=seed, inputShape=[16], hidden=hidden, layers=2, heads=1,
                                     ffn=2 * hidden, maxPositions=32, dataType=dtype, weightDataType=fmt,
                                     **kw).init(device=CPU)


def _quant_layers(net):
    return [(n, l) for n, l in net.layers_by_name.items() if l.wqKeys()]


def _twin_with_dequantised(net, fmt, **kw):
    twin = _lm(None, **kw)
    twin.setParams(net.params().clone())
    for (_, l), (_, t) in zip(_quant_layers(net), _quant_layers(twin)):
        for k in l.wqKeys():
            t.setParam(k, TN.wq_dequantize_reference(TN.wq_quantize_reference(l.params[k], fmt), l.params[k].dtype))
    return twin


@pytest.mark.parametrize("llama", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_time_step_reads_the_quantised_weights(fmt, llama):
    net = _lm(fmt, llama=llama)
    assert [n for n, _ in _quant_layers(net)] == ["decoder_0", "decoder_1", "output"]
    twin = _twin_with_dequantised(net, fmt, llama=llama)
    x = torch.randint(0, 77, (2, 6), generator=torch.Generator().manual_seed(1))
    full = net.output(x)[0].clone()
    for chunk in (x[:, :5], x[:, 5:]):                             # a prompt chunk, then one step
        got, want = net.rnnTimeStep(chunk)[0], twin.rnnTimeStep(chunk)[0]
        assert (got - want).abs().max() < 1e-12
    assert (got - full[:, :, 5:]).abs().max() > 1e-6, "rnnTimeStep reads the quantised copies"
    assert torch.equal(net.output(x)[0], full), "output() never sees them"
    net.rnnSetWeightDataType(None)
    net.rnnClearPreviousState()
    assert (net.rnnTimeStep(x)[0] - full).abs().max() < 1e-12


@pytest.mark.parametrize("fmt", FMTS)
def test_copies_follow_a_fit_step(fmt):
    net = _lm(fmt)
    x = torch.randint(0, 77, (2, 6), generator=torch.Generator().manual_seed(2))
    y = torch.nn.functional.one_hot(torch.roll(x, -1, 1), 77).permute(0, 2, 1).double()
    before = net.rnnTimeStep(x)[0].clone()
    net.fit([x], [y])
    net.rnnClearPreviousState()
    twin = _twin_with_dequantised(net, fmt)                        # from the NEW parameters
    got = net.rnnTimeStep(x)[0]
    assert (got - twin.rnnTimeStep(x)[0]).abs().max() < 1e-12
    assert (got - before).abs().max() > 1e-6


def test_refusals_name_the_layer_and_change_nothing():
    net = _lm(None)
    with pytest.raises(DL4JInvalidConfigException, match="fp8.*fp4.*int4"):
        net.rnnSetWeightDataType("int4")
    net.layers_by_name["decoder_1"].params["Wo"][3, 5] = float("nan")
    with pytest.raises(DL4JInvalidInputException, match="decoder_1.*TransformerEncoderLayer.*'Wo'"):
        net.rnnSetWeightDataType("fp8")
    odd = _lm(None, hidden=48)                                     # nIn = 48 of Wqkv, Wo, W1 and the output layer
    with pytest.raises(DL4JInvalidConfigException, match="decoder_0.*TransformerEncoderLayer.*'Wqkv'.*48"):
        odd.rnnSetWeightDataType("fp4")
    for n in (net, odd):
        assert all(l._wq_fmt is None for _, l in _quant_layers(n))
