"""Quantised mixture-of-experts experts off the GPU: an fp64 two-block sparse language model whose rnnTimeStep reads
the per-expert MXFP8 / MXFP4 copies (against the same network holding every expert's dequantised values), and the
refusals of rnnSetWeightDataType(..., experts=)."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException, DL4JInvalidInputException
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import transformer_native as TN

CPU = torch.device("cpu")
X = 4
LLAMA = dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu", positionEncoding="rotary")


def _lm(fmt=None, llama=False, hidden=64, ffn=64, experts=X):
    return TextGenerationTransformer(numLabels=77, seed=7, inputShape=[16], hidden=hidden, layers=2, heads=1, ffn=ffn,
                                     maxPositions=32, dataType=DataType.DOUBLE, nExperts=experts, nExpertsPerToken=2,
                                     expertWeightDataType=fmt, **(LLAMA if llama else {})).init(device=CPU)


def _blocks(net):
    return [l for l in net.layers_by_name.values() if l.wqExpertKeys()]


@pytest.mark.parametrize("llama", [False, True], ids=["gelu", "swiglu"])
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_time_step_reads_the_quantised_experts(fmt, llama):
    net, twin = _lm(fmt, llama), _lm(None, llama)
    # Freshly initialised experts add so little to the residual stream that fp8's 2^-4 relative rounding moves the
    # output probabilities (~1/77) by about 6e-7 in the pre-norm model: too little to tell which copy was read. Four
    # times the expert weights (a power of two: the codes stay, the scales move) gives the branch a trained model's say.
    for l in _blocks(net):
        for k in l.wqExpertKeys():
            l.setParam(k, l.params[k] * 4.0)
    twin.setParams(net.params().clone())
    assert len(_blocks(net)) == 2
    for l, t in zip(_blocks(net), _blocks(twin)):
        assert l.wqExpertKeys() == ("W1", "W2") and l._wq_fmt is None and l._wq_expert_fmt == fmt
        for k in l.wqExpertKeys():
            w = l.params[k].reshape(X, -1, l.params[k].shape[1])            # each expert quantised on its own
            deq = [TN.wq_dequantize_reference(TN.wq_quantize_reference(w[e], fmt), w.dtype) for e in range(X)]
            t.setParam(k, torch.cat(deq))
    x = torch.randint(0, 77, (2, 6), generator=torch.Generator().manual_seed(1))
    full = net.output(x)[0].clone()
    for chunk in (x[:, :5], x[:, 5:]):                                      # a 5-token chunk, then one step
        got, want = net.rnnTimeStep(chunk)[0], twin.rnnTimeStep(chunk)[0]
        assert (got - want).abs().max() < 1e-12
    assert (got - full[:, :, 5:]).abs().max() > 1e-6, "rnnTimeStep reads the quantised experts"
    assert torch.equal(net.output(x)[0], full), "output() never sees them"
    net.rnnSetWeightDataType(None)                                          # every call sets both formats
    net.rnnClearPreviousState()
    assert all(l._wq_expert_fmt is None for l in _blocks(net))
    assert (net.rnnTimeStep(x)[0] - full).abs().max() < 1e-12


def test_refusals_name_the_layer_and_change_nothing():
    with pytest.raises(DL4JInvalidConfigException, match="fp8.*fp4.*int4"):
        _lm().rnnSetWeightDataType(None, experts="int4")
    odd_in, odd_ffn, nan = _lm(hidden=48), _lm(ffn=48), _lm()
    with pytest.raises(DL4JInvalidConfigException, match="decoder_0.*TransformerEncoderLayer.*'W1'.*48"):
        odd_in.rnnSetWeightDataType(None, experts="fp4")
    with pytest.raises(DL4JInvalidConfigException, match="decoder_0.*TransformerEncoderLayer.*'W2'.*48"):
        odd_ffn.rnnSetWeightDataType(None, experts="fp8")
    nan.layers_by_name["decoder_1"].params["W2"][3 * 64 + 1, 5] = float("nan")       # in expert 3
    with pytest.raises(DL4JInvalidInputException, match="decoder_1.*TransformerEncoderLayer.*'W2'"):
        nan.rnnSetWeightDataType("fp8", experts="fp8")
    for n in (odd_in, odd_ffn, nan):
        assert all(l._wq_fmt is None and l._wq_expert_fmt is None for l in n.layers_by_name.values())


def test_a_dense_network_takes_the_expert_format_as_a_no_op():
    net = _lm(experts=None)
    x = torch.randint(0, 77, (2, 6), generator=torch.Generator().manual_seed(1))
    want = net.rnnTimeStep(x)[0].clone()
    net.rnnClearPreviousState()
    net.rnnSetWeightDataType(None, experts="fp8")
    assert not _blocks(net) and torch.equal(net.rnnTimeStep(x)[0], want)
