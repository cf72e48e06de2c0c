"""rnnSetWeightDataType("native") off the GPU: the value is accepted, unknown ones are still refused, and a CPU
network's rnnTimeStep gives the numbers it gives without a format (the skinny kernels' twin is the matmul path)."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer

CPU = torch.device("cpu")


def _lm(fmt=None, experts=None, **kw):
    return TextGenerationTransformer(numLabels=77, seed=7, inputShape=[16], hidden=48, layers=2, heads=1, ffn=96,
                                     maxPositions=32, dataType=DataType.DOUBLE, weightDataType=fmt,
                                     expertWeightDataType=experts, **kw).init(device=CPU)


LLAMA = dict(normalization="rms", normPlacement="pre", ffnActivation="swiglu", positionEncoding="rotary")


@pytest.mark.parametrize("kw", [{}, LLAMA, dict(nExperts=4, nExpertsPerToken=2), dict(nExperts=4, **LLAMA)],
                         ids=["bert", "llama", "bert-moe", "llama-moe"])
def test_native_is_accepted_and_changes_no_number(kw):
    net, plain = _lm("native", "native", **kw), _lm(**kw)         # hidden 48: "native" has no nIn % 32 condition
    x = torch.randint(0, 77, (2, 6), generator=torch.Generator().manual_seed(1))
    for chunk in (x[:, :4], x[:, 4:5], x[:, 5:6]):
        assert torch.equal(net.rnnTimeStep(chunk)[0], plain.rnnTimeStep(chunk)[0])
    net.rnnClearPreviousState()
    net.rnnSetWeightDataType("native", experts=None)              # independent per argument
    net.rnnSetWeightDataType(None, experts="native")
    with pytest.raises(DL4JInvalidConfigException, match="fp8.*fp4.*native.*int4"):
        net.rnnSetWeightDataType("int4")
    with pytest.raises(DL4JInvalidConfigException, match="experts.*native.*int4"):
        net.rnnSetWeightDataType("native", experts="int4")
