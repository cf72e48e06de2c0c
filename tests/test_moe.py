"""Mixture-of-experts feed-forward on the CPU (``nExperts`` / ``nExpertsPerToken`` on TransformerEncoderLayer): the
configuration and its refusals, serialisation, the routing contract of ``moe_route_reference`` against a per-token
loop in fp64, the layer's forward against the explicit per-token sum over experts, the fp64 gradient check, streaming
and generation. The kernels are tested in tests/test_gpu_moe.py against the same twins."""
import io
import json
import math

import pytest
import torch
import torch.nn.functional as F_

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.exceptions import DL4JInvalidConfigException
from deeplearning4j_amd.gradientcheck import checkGradients
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import transformer_native as TN
from deeplearning4j_amd.utils.model_serializer import ModelSerializer

V, E, H, F, T, MB, X, K = 11, 16, 4, 24, 5, 2, 4, 2
G = TN.MOE_ROW_TILE
LLAMA = ("rms", "pre", "swiglu")
BERT = ("layer", "post", "gelu")
STYLES = [LLAMA, ("rms", "pre", "gelu"), ("layer", "post", "swiglu"), BERT]
STYLE_IDS = ["rms-pre-swiglu", "rms-pre-gelu", "layer-post-swiglu", "layer-post-gelu"]


def _builder(dt=DataType.DOUBLE, std=0.5, seed=7):
    return (NeuralNetConfiguration.Builder().seed(seed).dataType(dt).updater(NoOp())
            .weightInit(NormalDistribution(0.0, std)))


def _enc(style=LLAMA, x=X, k=K, name=None, f=F):
    norm, place, act = style
    b = (TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(f).causal(True)
         .positionEncoding("rotary").layerNormEps(1e-5).normalization(norm).normPlacement(place).ffnActivation(act))
    if name:
        b = b.name(name)
    if x is not None:
        b = b.nExperts(x)
    if k is not None:
        b = b.nExpertsPerToken(k)
    return b.build()


def _lm(dt=DataType.DOUBLE, style=LLAMA, x=X, k=K, t=T, seed=7, std=0.5, f=F):
    """tokens -> embeddings -> two causal sparse blocks (-> final RMSNorm for a pre-norm stack) -> softmax"""
    g = _builder(dt, std, seed).graphBuilder()
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(t + 2).inputLength(t)
               .positionEmbeddings(False).build(), "tokens")
    g.addLayer("enc0", _enc(style, x, k, f=f), "emb")
    g.addLayer("enc1", _enc(style, x, k, f=f), "enc0")
    last = "enc1"
    if style[1] == "pre":
        g.addLayer("norm", RMSNormalization.Builder().nIn(E).nOut(E).build(), last)
        last = "norm"
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V)
               .build(), last)
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device="cpu")
    return net


def _tokens(mb=MB, t=T, seed=0):
    return torch.randint(0, V, (mb, t), generator=torch.Generator().manual_seed(seed))


def _labels(t=T, seed=2, dt=torch.float64):
    y = torch.zeros(MB, V, t, dtype=dt)
    y.scatter_(1, torch.randint(0, V, (MB, 1, t), generator=torch.Generator().manual_seed(seed)), 1.0)
    return y


# ------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("x", [0, 65, 2.5, True, "4"])
def test_a_bad_number_of_experts_is_refused_naming_the_layer(x):
    with pytest.raises(DL4JInvalidConfigException, match="TransformerEncoderLayer.*nExperts"):
        _enc(x=x)
    with pytest.raises(DL4JInvalidConfigException, match="TransformerEncoderLayer 'blk'.*nExperts"):
        _enc(x=x, name="blk")


@pytest.mark.parametrize("x,k", [(4, 0), (4, 5), (16, 9), (4, 1.5), (None, 1), (None, 3)])
def test_a_bad_number_of_experts_per_token_is_refused_naming_the_layer(x, k):
    with pytest.raises(DL4JInvalidConfigException, match="TransformerEncoderLayer 'blk'.*nExpertsPerToken"):
        _enc(x=x, k=k, name="blk")


def test_the_limits_are_accepted_and_the_decoder_block_does_not_take_the_fields():
    assert _enc(x=64, k=8).nExperts == 64 and _enc(x=1, k=1).nExpertsPerToken == 1
    assert _enc(x=None, k=2).nExperts is None and _enc(x=None, k=None).nExpertsPerToken == 2
    for field in ("nExperts", "nExpertsPerToken"):
        with pytest.raises((AttributeError, DL4JInvalidConfigException), match=f"TransformerDecoderLayer.*{field}"):
            getattr(TransformerDecoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F), field)(2).build()


# ------------------------------------------------------------------------------------------------ serialisation
def test_conf_fields_round_trip_and_the_defaults_leave_the_json_alone():
    dense = _enc(x=None, k=None)
    text = dense.toJson()
    assert "nExperts" not in text and "nExpertsPerToken" not in text
    assert TransformerEncoderLayer.fromJson(text) == dense
    sparse = _enc(x=8, k=3)
    d = json.loads(sparse.toJson())
    assert '"nExperts": 8' in sparse.toJson() and '"nExpertsPerToken": 3' in sparse.toJson(), d
    back = TransformerEncoderLayer.fromJson(sparse.toJson())
    assert back == sparse and back.nExperts == 8 and back.nExpertsPerToken == 3
    two = _enc(x=8, k=2)                                    # k at its default stays out, the experts do not
    assert "nExpertsPerToken" not in two.toJson() and '"nExperts": 8' in two.toJson()
    assert TransformerEncoderLayer.fromJson(two.toJson()) == two


def test_network_conf_round_trips_through_json_and_yaml():
    net = _lm()
    text = net.conf.toJson()
    assert text.count('"nExperts": 4') == 2
    again = ComputationGraphConfiguration.fromJson(text)
    assert again.toJson() == text
    y = net.conf.toYaml()
    assert "nExperts: 4" in y
    assert ComputationGraphConfiguration.fromYaml(y).toJson() == text


@pytest.mark.parametrize("style", [LLAMA, BERT], ids=["swiglu", "gelu"])
def test_parameter_shapes_and_count(style):
    conf = _enc(style)
    f1 = 2 * F if style[2] == "swiglu" else F
    specs = {p.key: p for p in conf.param_specs()}
    shapes = {k: tuple(p.shape) for k, p in specs.items()}
    assert shapes["Wr"] == (E, X) and shapes["W1"] == (X * E, f1) and shapes["b1"] == (X, f1)
    assert shapes["W2"] == (X * F, E) and shapes["b2"] == (X, E)
    assert list(specs).index("Wr") == list(specs).index("W1") - 1
    assert not conf.is_bias("Wr") and conf.is_bias("b1") and conf.is_bias("b2")
    net = _lm(style=style)
    n_norm = 2 * E if style[0] == "rms" else 4 * E
    per_block = E * 3 * E + 3 * E + E * E + E + n_norm + E * X + X * (E * f1 + f1 + F * E + E)
    assert net.layers_by_name["enc0"].params["W1"].shape == (X * E, f1)
    assert sum(p.numel() for p in net.layers_by_name["enc0"].params.values()) == per_block
    # the weight initialisation sees one expert's fans: N(0, 0.5) here, so only the spread can be checked
    w1 = net.layers_by_name["enc0"].params["W1"]
    assert 0.3 < float(w1.std()) < 0.7 and float(net.layers_by_name["enc0"].params["b1"].abs().max()) == 0.0


def test_model_save_and_load_round_trips_the_experts():
    net = _lm(DataType.FLOAT)
    gen = torch.Generator().manual_seed(6)
    net.setParams(net.params() + 0.1 * torch.randn(net.numParams(), generator=gen))
    buf = io.BytesIO()
    ModelSerializer.writeModel(net, buf, True)
    buf.seek(0)
    back = ModelSerializer.restoreComputationGraph(buf, True)
    assert back.conf.toJson() == net.conf.toJson()
    assert torch.equal(back.params(), net.params())
    for key, p in net.layers_by_name["enc1"].params.items():
        assert torch.equal(back.layers_by_name["enc1"].params[key], p), key
    x = _tokens()
    assert torch.equal(back.output(x)[0], net.output(x)[0])


# ------------------------------------------------------------------------------------------------ routing contract
def _route_loop(logits, k):
    """The contract, token by token in Python floats (fp64): -> idx, gate, and the plan arrays as lists."""
    N, X_ = logits.shape
    idx, gate = [], []
    for n in range(N):
        l = [float(v) for v in logits[n]]
        order = sorted(range(X_), key=lambda e: (-l[e], e))[:k]
        ex = [math.exp(l[e] - l[order[0]]) for e in order]
        s = sum(ex)
        idx.append(order)
        gate.append([v / s for v in ex])
    cnt = [sum(e in row for row in idx) for e in range(X_)]
    off = [0]
    for e in range(X_):
        off.append(off[-1] + -(-cnt[e] // G) * G)
    rows = -(-(N * k + X_ * (G - 1)) // G) * G
    row_of = [[None] * k for _ in range(N)]
    src_of = [-1] * rows
    fill = list(off[:-1])
    for n in range(N):                                      # (token, choice) ascending inside every segment
        for j in range(k):
            e = idx[n][j]
            row_of[n][j] = fill[e]
            src_of[fill[e]] = n * k + j
            fill[e] += 1
    tile = []
    for t in range(rows // G):
        es = [e for e in range(X_) if off[e] <= t * G < off[e + 1]]
        tile.append(es[0] if es else -1)
    return idx, gate, cnt, off, row_of, src_of, tile, rows


@pytest.mark.parametrize("n,x,k,ties", [(37, 4, 2, False), (37, 4, 2, True), (300, 8, 3, True), (5, 64, 8, True),
                                        (3, 4, 1, False), (1, 8, 2, False), (140, 2, 2, True)])
def test_route_reference_against_a_per_token_loop(n, x, k, ties):
    g = torch.Generator().manual_seed(1000 * n + 10 * x + k)
    logits = torch.randn(n, x, generator=g, dtype=torch.float64)
    if ties:                                                # planted equal logits, the top ones among them
        logits[::3] = torch.round(logits[::3])
        logits[1::5, : max(2, x // 2)] = 2.0
    idx, gate, cnt, off, row_of, src_of, tile, rows = _route_loop(logits, k)
    plan, got = TN.moe_route_reference(logits, k)
    assert (plan.N, plan.k, plan.X, plan.rows) == (n, k, x, rows) and rows == TN.moe_rows(n, k, x)
    for name, want in (("idx", idx), ("cnt", cnt), ("off", off), ("row_of", row_of), ("src_of", src_of),
                       ("tile_expert", tile)):
        t = getattr(plan, name)
        assert t.dtype == torch.int32 and t.tolist() == want, name
    assert (got - torch.tensor(gate, dtype=torch.float64)).abs().max() < 1e-15
    assert (got.sum(1) - 1).abs().max() < 1e-15
    # the same decisions in fp32 on the same (fp32-representable) logits
    l32 = logits.float()
    p32, g32 = TN.moe_route_reference(l32, k)
    w = _route_loop(l32.double(), k)
    assert p32.idx.tolist() == w[0] and p32.src_of.tolist() == w[5]
    assert ((g32.double() - torch.tensor(w[1])).abs() <= 4 * 2.0 ** -24 * torch.tensor(w[1])).all()


def test_all_equal_logits_give_the_first_experts_with_equal_weights():
    for x, k in ((4, 2), (8, 3), (64, 8), (3, 1)):
        plan, gate = TN.moe_route_reference(torch.full((6, x), 0.25), k)
        assert plan.idx.tolist() == [list(range(k))] * 6
        assert torch.equal(gate, torch.full((6, k), 1.0 / k))
        assert plan.cnt.tolist() == [6] * k + [0] * (x - k)


def test_the_twins_of_the_permutation_kernels_on_a_small_plan():
    g = torch.Generator().manual_seed(4)
    n, x, k, e = 9, 3, 2, 8
    plan, gate = TN.moe_route_reference(torch.randn(n, x, generator=g, dtype=torch.float64), k)
    v = torch.randn(n, e, generator=g, dtype=torch.float64)
    xp = TN.moe_gather_reference(v, plan)
    src = plan.src_of.tolist()
    for r in range(plan.rows):
        want = v[src[r] // k] if src[r] >= 0 else torch.zeros(e, dtype=torch.float64)
        assert torch.equal(xp[r], want), r
    xs = TN.moe_gather_reference(v, plan, gate)
    for r in range(plan.rows):
        if src[r] >= 0:
            assert torch.equal(xs[r], v[src[r] // k] * gate.reshape(-1)[src[r]])
    b = torch.randn(x, e, 5, generator=g, dtype=torch.float64)
    bias = torch.randn(x, 5, generator=g, dtype=torch.float64)
    c = TN.gemm_grouped_reference(xp, b, bias, plan)
    te = plan.tile_expert.tolist()
    for r in range(plan.rows):
        ex = te[r // G]
        want = xp[r] @ b[ex] + bias[ex] if ex >= 0 else torch.zeros(5, dtype=torch.float64)
        assert (c[r] - want).abs().max() < 1e-12
    y = TN.moe_combine_reference(c, plan, gate, None)
    row_of = plan.row_of.tolist()
    for t in range(n):
        want = sum(gate[t, j] * c[row_of[t][j]] for j in range(k))
        assert (y[t] - want).abs().max() < 1e-12
    dw = torch.empty(x * e, 5, dtype=torch.float64)
    TN.gemm_grouped_wgrad_reference(xp, c, plan, dw)
    bs = torch.empty(x, 5, dtype=torch.float64)
    TN.moe_segment_colsum_reference(c, plan, bs)
    off, cnt = plan.off.tolist(), plan.cnt.tolist()
    for ex in range(x):
        seg = slice(off[ex], off[ex] + cnt[ex])
        assert (dw[ex * e:(ex + 1) * e] - xp[seg].t() @ c[seg]).abs().max() < 1e-12
        assert (bs[ex] - c[seg].sum(0)).abs().max() < 1e-12
    # route backward against autograd through the gate formula
    lg = torch.randn(n, x, generator=g, dtype=torch.float64, requires_grad=True)
    plan, gate = TN.moe_route_reference(lg.detach(), k)
    dgate = torch.randn(n, k, generator=g, dtype=torch.float64)
    chosen = lg.gather(1, plan.idx.long())
    (torch.softmax(chosen, 1) * dgate).sum().backward()
    dl = TN.moe_route_bwd_reference(plan, gate, dgate, torch.float64)
    assert (dl - lg.grad).abs().max() < 1e-14


# ------------------------------------------------------------------------------------------------ layer forward
def _act(z, swiglu):
    return TN.swiglu_reference(z) if swiglu else F_.gelu(z)


def _ffn_per_token(n, P, x, k, swiglu):
    """f2[t] = sum_j g_j * FFN_{e_j}(n[t]), token by token."""
    Fh = P["W2"].shape[0] // x
    e_in = n.shape[1]
    out = torch.zeros_like(n)
    for t in range(n.shape[0]):
        l = n[t] @ P["Wr"]
        order = sorted(range(x), key=lambda e: (-float(l[e]), e))[:k]
        ex = torch.exp(l[order] - l[order[0]])
        gate = ex / ex.sum()
        for j, e in enumerate(order):
            z = n[t] @ P["W1"][e * e_in:(e + 1) * e_in] + P["b1"][e]
            out[t] += gate[j] * (_act(z, swiglu) @ P["W2"][e * Fh:(e + 1) * Fh] + P["b2"][e])
    return out


@pytest.mark.parametrize("style", STYLES, ids=STYLE_IDS)
def test_the_feed_forward_equals_the_per_token_sum_over_experts(style):
    net = _lm(style=style)
    gen = torch.Generator().manual_seed(8)
    net.setParams(net.params() + 0.3 * torch.randn(net.numParams(), generator=gen, dtype=torch.float64))
    layer = net.layers_by_name["enc0"]
    P = layer.params
    n = torch.randn(MB * T, E, generator=gen, dtype=torch.float64)
    want = _ffn_per_token(n, P, X, K, style[2] == "swiglu")
    f2, ctx = layer._moe_fwd(n)
    assert (f2 - want).abs().max() < 1e-12
    ref = TN.moe_ffn_reference(n, P["Wr"], P["W1"], P["b1"], P["W2"], P["b2"], K, style[2] == "swiglu")
    assert (ref - want).abs().max() < 1e-12
    acc = torch.randn(MB * T, E, generator=gen, dtype=torch.float64)
    assert (layer._moe_fwd(n, acc=acc.clone())[0] - (want + acc)).abs().max() < 1e-12
    plan = ctx[0]
    assert plan.rows == TN.moe_rows(MB * T, K, X) and int(plan.cnt.sum()) == MB * T * K


@pytest.mark.parametrize("style", STYLES, ids=STYLE_IDS)
def test_the_whole_block_uses_the_sparse_feed_forward(style):
    """The block's output moves with one column of the experts' second bias (a uniform shift of all of them would
    vanish in the post-norm block's LayerNorm: the gates sum to one)."""
    net = _lm(style=style)
    x = _tokens()
    base = net.output(x)[0].clone()
    with torch.no_grad():
        net.layers_by_name["enc1"].params["b2"][:, 0].add_(0.5)
    net._params_changed()
    assert (net.output(x)[0] - base).abs().max() > 1e-6


def test_one_expert_with_the_dense_weights_equals_the_dense_block():
    """nExperts = 1, k = 1: the gate is exp(0) / exp(0) = 1 exactly and the expert's matrices are the dense block's, so
    the outputs differ only by fp64 reassociation inside the matrix products (the sparse path multiplies padded row
    tiles): a few ulp of values of order 1..10, bound 1e-12."""
    for style in (LLAMA, BERT):
        dense, sparse = _lm(style=style, x=None, k=None), _lm(style=style, x=1, k=1)
        for name in ("emb", "enc0", "enc1", "out"):
            for key, p in sparse.layers_by_name[name].params.items():
                if key == "Wr":
                    continue
                with torch.no_grad():
                    p.copy_(dense.layers_by_name[name].params[key].reshape(p.shape))
        sparse._params_changed()
        x = _tokens()
        a, b = dense.output(x)[0], sparse.output(x)[0]
        assert (a - b).abs().max() < 1e-12, style


# ------------------------------------------------------------------------------------------------ gradients
def _router_gaps(net, x, k=K):
    """The smallest gap between the k-th and the (k+1)-th router logit over every token of every sparse block."""
    gaps = []
    seen = {}

    def spy(layer):
        orig = layer._moe_fwd

        def fwd(n, acc=None):
            l = torch.sort(n @ layer.params["Wr"].to(n.dtype), dim=1, descending=True).values
            seen.setdefault(id(layer), []).append(float((l[:, k - 1] - l[:, k]).min()))
            return orig(n, acc)
        layer._moe_fwd = fwd
        return orig
    saved = {name: spy(net.layers_by_name[name]) for name in ("enc0", "enc1")}
    net.output(x)
    for name, orig in saved.items():
        del net.layers_by_name[name]._moe_fwd
    for v in seen.values():
        gaps.extend(v)
    return min(gaps)


GRAD_SEED = 7


def _moe_indices(net, layer, f):
    """Flat positions of the router, both expert biases, and four rows of one expert's slab of W1 and of W2."""
    from deeplearning4j_amd.gradientcheck import paramIndices
    idx = []
    for key in ("Wr", "b1", "b2"):
        idx += paramIndices(net, layer, key)
    w1, w2 = paramIndices(net, layer, "W1"), paramIndices(net, layer, "W2")
    f1 = len(w1) // (X * E)
    idx += w1[(1 * E + 3) * f1:(1 * E + 7) * f1]            # expert 1, input rows 3..6
    idx += w2[(2 * f + 1) * E:(2 * f + 5) * E]              # expert 2, hidden rows 1..4
    return idx


GRAD_F = 8


def test_gradient_check_of_a_two_block_model():
    """E = 16, X = 4, k = 2, T = 5, mb = 2 (ffnSize 8). The check perturbs by 1e-6; the seed is one for which every
    token's k-th / (k+1)-th logit gap is at least 1e-3, so no routing decision flips inside it. The model has about
    6000 parameters and a check of all of them takes minutes, so ``checkGradients`` runs twice: on every entry of Wr,
    b1 and b2 and four rows of one expert's W1 and W2 of the first block, and on 40 positions drawn from the whole
    model."""
    net = _lm(seed=GRAD_SEED, f=GRAD_F)
    x, y = _tokens(), _labels()
    gap = _router_gaps(net, x)
    assert gap >= 1e-3, gap
    idx = _moe_indices(net, "enc0", GRAD_F)
    assert len(idx) == E * X + X * 2 * GRAD_F + X * E + 4 * 2 * GRAD_F + 4 * E
    assert checkGradients(net, input=[x], labels=[y], print_results=True, indices=idx)
    assert checkGradients(net, input=[x], labels=[y], print_results=True, subset=40)
    for name in ("enc0", "enc1"):
        g = net.layers_by_name[name].grads
        assert all(float(g[k_].abs().sum()) > 0 for k_ in ("Wr", "W1", "b1", "W2", "b2"))


@pytest.mark.parametrize("style", [("layer", "post", "gelu"), ("layer", "post", "swiglu"), ("rms", "pre", "gelu")],
                         ids=["layer-post-gelu", "layer-post-swiglu", "rms-pre-gelu"])
def test_gradient_check_of_the_other_block_styles(style):
    net = _lm(style=style, seed=GRAD_SEED, f=GRAD_F)
    x = _tokens()
    assert _router_gaps(net, x) >= 1e-3
    idx = _moe_indices(net, "enc1", GRAD_F)[::3]
    assert checkGradients(net, input=[x], labels=[_labels()], print_results=True, indices=idx)
    assert checkGradients(net, input=[x], labels=[_labels()], print_results=True, subset=30)


# ------------------------------------------------------------------------------------------------ streaming, generation
def _stream(net, x, chunks):
    outs, t = [], 0
    for n in chunks:
        outs.append(net.rnnTimeStep(x[:, t:t + n])[0])
        t += n
    assert t == x.shape[1]
    return torch.cat(outs, 2)


@pytest.mark.parametrize("style", [LLAMA, BERT], ids=["rms-pre-swiglu", "layer-post-gelu"])
def test_chunked_time_step_equals_output(style):
    net = _lm(style=style, t=10)
    x = _tokens(t=10)
    ref = net.output(x)[0]
    net.rnnClearPreviousState()
    assert (_stream(net, x, (5, 1, 1, 3)) - ref).abs().max() < 1e-10
    net.rnnClearPreviousState()
    assert (_stream(net, x, (1,) * 10) - ref).abs().max() < 1e-10


def _zoo(**kw):
    return TextGenerationTransformer(numLabels=V, inputShape=[T], hidden=E, layers=2, heads=H, ffn=F,
                                     positionEncoding="rotary", normalization="rms", normPlacement="pre",
                                     ffnActivation="swiglu", **kw)


def test_the_zoo_model_generates_greedy_and_seeded():
    net = _zoo(nExperts=4).init(device="cpu")
    for i in range(2):
        c = net.layers_by_name[f"decoder_{i}"].conf
        assert c.nExperts == 4 and c.nExpertsPerToken == 2
        assert "Wr" in net.layers_by_name[f"decoder_{i}"].params
    p0 = net.params().clone()
    net.fit([_tokens()], [_labels(dt=torch.float32)])
    assert torch.isfinite(net.params()).all() and not torch.equal(p0, net.params())
    prompt = _tokens(t=4, seed=9)
    greedy = net.generate(prompt, maxNewTokens=12)
    assert greedy.tokens.shape == (MB, 12) and torch.equal(net.generate(prompt, maxNewTokens=12).tokens, greedy.tokens)
    assert torch.equal(net.generate(prompt, maxNewTokens=12, pinPositions=True).tokens, greedy.tokens)
    a = net.generate(prompt, maxNewTokens=12, doSample=True, temperature=1.3, seed=11)
    b = net.generate(prompt, maxNewTokens=12, doSample=True, temperature=1.3, seed=11)
    c = net.generate(prompt, maxNewTokens=12, doSample=True, temperature=1.3, seed=12)
    assert torch.equal(a.tokens, b.tokens) and not torch.equal(a.tokens, c.tokens)
    net.rnnClearPreviousState()
    p = net.rnnTimeStep(prompt)[0][:, :, -1]
    for t in range(12):
        tok = p.argmax(1)
        assert torch.equal(tok, greedy.tokens[:, t])
        p = net.rnnTimeStep(tok.reshape(MB, 1))[0][:, :, -1]


def test_a_per_block_sequence_builds_sparse_and_dense_blocks():
    net = _zoo(nExperts=[4, None], nExpertsPerToken=1).init(device="cpu")
    c0, c1 = (net.layers_by_name[f"decoder_{i}"].conf for i in range(2))
    assert (c0.nExperts, c0.nExpertsPerToken) == (4, 1) and (c1.nExperts, c1.nExpertsPerToken) == (None, 2)
    assert "Wr" in net.layers_by_name["decoder_0"].params and "Wr" not in net.layers_by_name["decoder_1"].params
    assert net.layers_by_name["decoder_1"].params["W1"].shape == (E, 2 * F)
    assert net.generate(_tokens(t=3), maxNewTokens=4).tokens.shape == (MB, 4)
    with pytest.raises(DL4JInvalidConfigException, match="nExperts has 3 entries for 2 blocks"):
        _zoo(nExperts=[4, None, 4]).conf()
    assert "nExperts" not in _zoo().conf().toJson()
