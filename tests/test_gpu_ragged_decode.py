"""Ragged batches on the GPU: the key/value append, the decode attention and the BERT embedding with a per-row
shortfall array (csrc/attention_decode.hip, csrc/nn_misc.hip) against the fp32 reference of every row on its own
sequence, the key splits (accuracy, reproducibility, bitwise equality with the uniform kernel on the row alone), and
rnnTrimState / generate(promptLengths=...) on top of them (bf16 GPU against fp32 CPU, no fallback, no torch compute
kernel in a steady-state step). Pattern, error measure and bounds: tests/test_gpu_attention_decode.py."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.ops import nn_misc
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(4, 2, 64), (3, 3, 128)]
# Tn = 1: a single key, both sides of the 64-key block edge, whole blocks; Tn > 1: a ragged 16-query wave, a chunk
# crossing a wave, a chunk crossing a 64-query tile. The largest position of a launch is its upper bound (shortfall 0).
POSITIONS = {
    (1, 4): [(191, 1, 63, 64), (128, 65, 64, 128)],
    (1, 3): [(191, 1, 63), (128, 64, 65)],
    (3, 4): [(60, 50, 10, 60)], (17, 4): [(60, 50, 10, 60)], (65, 4): [(60, 50, 10, 60)],
    (3, 3): [(60, 50, 10)], (17, 3): [(60, 50, 10)], (65, 3): [(60, 50, 10)],
}
CASES = [(B, H, D, Tn, ps) for (B, H, D) in SHAPES for Tn in (1, 3, 17, 65) for ps in POSITIONS[(Tn, B)]]


def _err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


@functools.lru_cache(maxsize=None)
def _row(dt, H, D, pos, Tn, seed):
    """(qkv [1, pos+Tn, 3E] in dt on the CPU, oracle [1, Tn, E]): attention_reference in fp32 on the row's own whole
    sequence built from the rounded inputs, causal, last Tn rows. Computed once per row and never modified."""
    g = torch.Generator().manual_seed(seed * 7919 + H * 100 + D + 7 * pos + Tn)
    qkv = (torch.randn(1, pos + Tn, 3 * H * D, generator=g) * 0.8).to(dt)
    ref = TN.attention_reference(qkv.float(), H, None, True)[:, pos:].contiguous()
    return qkv, ref


def _ragged_cache(dt, H, D, Tn, poss):
    """NaN-filled cache with every row's own history, the new chunk [B, Tn, 3E], the shortfall array against
    max(poss) and the per-row oracle. The history goes in with the uniform append on the row's slice."""
    B, pos = len(poss), max(poss)
    E = H * D
    rows = [_row(dt, H, D, p, Tn, b) for b, p in enumerate(poss)]
    tcap = ((pos + Tn) // 64 + 1) * 64 + 64
    kv = torch.full((B, tcap, 2 * E), float("nan"), dtype=dt, device=DEV)
    for b, p in enumerate(poss):
        if p:
            assert TN.attn_kv_append(rows[b][0][:, :p].to(DEV).contiguous(), kv[b:b + 1], H, 0) is not None
    new = torch.cat([rows[b][0][:, p:] for b, p in enumerate(poss)]).to(DEV).contiguous()
    short = torch.tensor([pos - p for p in poss], dtype=torch.int32, device=DEV)
    return kv, new, short, [r[1] for r in rows]


@pytest.mark.parametrize("B,H,D,Tn,poss", CASES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ragged_append_and_decode_match_every_rows_reference(dt, B, H, D, Tn, poss):
    kv, new, short, refs = _ragged_cache(dt, H, D, Tn, poss)
    pos, E = max(poss), H * D
    before = kv.clone()
    assert TN.attn_kv_append(new, kv, H, pos, short=short) is kv
    out = TN.attn_decode(new, kv, H, pos, short=short)
    assert out is not None and out.dtype == dt and out.shape == (B, Tn, E)
    assert torch.isfinite(out).all(), "a row past a batch row's own length reached the products"
    for b, p in enumerate(poss):
        assert torch.isnan(kv[b, p + Tn:]).all(), f"row {b}: the append wrote past {p} + {Tn}"
        assert torch.equal(kv[b, p:p + Tn], new[b, :, E:]), f"row {b}: the new keys / values are not at {p}"
        assert torch.equal(kv[b, :p], before[b, :p]), f"row {b}: the append changed the history"
        e = _err(out[b:b + 1], refs[b])
        print(f"ragged decode {dt} H={H} D={D} Tn={Tn} row {b} at {p} of {pos}: err {e:.3e}")
        assert e < 2e-2


def test_the_append_clamps_whatever_the_array_holds():
    """A shortfall outside [0, pos] is clamped: no write leaves rows [0, pos + Tn) of its own batch row."""
    B, H, D, Tn, pos, dt = 3, 2, 64, 3, 20, torch.bfloat16
    E = H * D
    g = torch.Generator().manual_seed(2)
    new = torch.randn(B, Tn, 3 * E, generator=g).to(dt).to(DEV)
    kv = torch.full((B, 64, 2 * E), float("nan"), dtype=dt, device=DEV)
    hist = torch.randn(pos, 2 * E, generator=g).to(dt).to(DEV)
    kv[0, :pos] = hist                                           # row 0 clamps to shortfall 0: it has a history
    short = torch.tensor([-5, 1000, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    assert TN.attn_kv_append(new, kv, H, pos, short=short) is kv
    for b, p in enumerate((pos, 0, 0)):
        assert torch.equal(kv[b, p:p + Tn], new[b, :, E:])
        assert torch.isnan(kv[b, p + Tn:]).all()
    assert torch.equal(kv[0, :pos], hist)
    assert torch.isfinite(TN.attn_decode(new, kv, H, pos, short=short)).all()
    assert TN.attn_kv_append(new, kv, H, pos, short=short.long()) is None       # not int32: refused
    assert TN.attn_decode(new, kv, H, pos, short=short[:2].contiguous()) is None  # not one entry per row


@pytest.mark.parametrize("H,D", [(2, 64), (3, 128)])
def test_ragged_decode_splits(H, D):
    """Upper bound 300 keys, rows of 300 / 257 / 70 / 1 keys (5, 5, 2, 1 key blocks), one new query per row."""
    dt, Tn, lens = torch.bfloat16, 1, (300, 257, 70, 1)
    poss = tuple(n - Tn for n in lens)
    pos = max(poss)
    kv, new, short, refs = _ragged_cache(dt, H, D, Tn, poss)
    assert TN.attn_kv_append(new, kv, H, pos, short=short) is kv
    for splits in (1, 2, 3, 5, 64):
        a = TN.attn_decode(new, kv, H, pos, splits=splits, short=short)
        b = TN.attn_decode(new, kv, H, pos, splits=splits, short=short)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"splits={splits} is not reproducible"
        for r, (p, n) in enumerate(zip(poss, lens)):
            e = _err(a[r:r + 1], refs[r])
            print(f"splits={splits} H={H} D={D} row {r} ({n} keys): err {e:.3e}")
            assert e < 2e-2
            if splits <= (n + 63) // 64:
                alone = TN.attn_decode(new[r:r + 1].contiguous(), kv[r:r + 1], H, p, splits=splits)
                assert torch.equal(a[r:r + 1], alone), f"splits={splits} row {r}: not the uniform kernel's bits"


@pytest.mark.parametrize("Tn", [1, 17])
@pytest.mark.parametrize("B,H,D", SHAPES)
def test_zero_shortfall_is_the_uniform_kernel_bitwise(B, H, D, Tn):
    dt, pos = torch.bfloat16, 300
    kv, new, short, _ = _ragged_cache(dt, H, D, Tn, (pos,) * B)
    assert int(short.abs().sum()) == 0
    kv2 = kv.clone()
    assert TN.attn_kv_append(new, kv, H, pos, short=short) is kv and TN.attn_kv_append(new, kv2, H, pos) is kv2
    assert torch.equal(kv[:, :pos + Tn], kv2[:, :pos + Tn]) and torch.isnan(kv[:, pos + Tn:]).all()
    for splits in (None, 1, 3, 5):
        assert torch.equal(TN.attn_decode(new, kv, H, pos, splits=splits, short=short),
                           TN.attn_decode(new, kv, H, pos, splits=splits))


# ------------------------------------------------------------------------------------------------ embedding
def _check_embed(got, want, dtype):
    """fp32 inputs: the kernel's sum is the torch sum bit for bit (the same two fp32 additions in the same order);
    16-bit inputs: within the tolerances of tests/test_gpu_bert_embed.py."""
    if dtype == torch.float32:
        assert torch.equal(got, want)
    else:
        tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
        torch.testing.assert_close(got.float(), want, rtol=tol, atol=tol * 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_ragged_bert_embedding(dtype):
    B, T, E, Vw, P, pos = 5, 3, 72, 13, 40, 20
    g = torch.Generator().manual_seed(4)
    Ww, Wp, Wt = (torch.randn(n, E, generator=g).to(dtype).to(DEV) for n in (Vw, P, 2))
    idx = torch.randint(0, Vw, (B, T), generator=g).to(DEV)
    short = torch.tensor([0, 20, 7, 19, 3], dtype=torch.int32, device=DEV)
    got = nn_misc.bert_embed_forward(Ww, Wp, Wt, idx, pos, short)
    assert got is not None and got.shape == (B * T, E) and got.dtype == dtype
    rows = ((pos - short.long()).reshape(B, 1) + torch.arange(T, device=DEV).reshape(1, T)).reshape(-1)
    _check_embed(got, Ww.float()[idx.reshape(-1)] + Wp.float()[rows] + Wt.float()[0].reshape(1, -1), dtype)
    zero = torch.zeros(B, dtype=torch.int32, device=DEV)
    assert torch.equal(nn_misc.bert_embed_forward(Ww, Wp, Wt, idx, pos, zero),
                       nn_misc.bert_embed_forward(Ww, Wp, Wt, idx, pos))
    # positions are clamped into the table whatever the array holds
    wild = torch.tensor([-100, 1000, 2 ** 31 - 1, -2 ** 31, 21], dtype=torch.int32, device=DEV)
    got = nn_misc.bert_embed_forward(Ww, Wp, Wt, idx, pos, wild)
    rows = ((pos - wild.long()).reshape(B, 1) + torch.arange(T, device=DEV).reshape(1, T)).clamp(0, P - 1).reshape(-1)
    _check_embed(got, Ww.float()[idx.reshape(-1)] + Wp.float()[rows] + Wt.float()[0].reshape(1, -1), dtype)


# ------------------------------------------------------------------------------------------------ network
TP, LENS, STEPS, VOC = 70, (70, 64, 63, 5), 6, 11


def _lm_graph(dt, device, maxp=TP + STEPS + 2, V=VOC, E=128, H=2, F=24):
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.05)).graphBuilder())
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(maxp).inputLength(TP).build(), "tokens")
    g.addLayer("enc0", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True).build(),
               "emb")
    g.addLayer("enc1", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True).build(),
               "enc0")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V)
               .build(), "enc1")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device=device)
    return net


@functools.lru_cache(maxsize=None)
def _nets():
    gpu = _lm_graph(DataType.BFLOAT16, DEV)
    cpu = _lm_graph(DataType.FLOAT, torch.device("cpu"))
    with torch.no_grad():
        cpu.flattenedParams.copy_(gpu.flattenedParams.cpu())
    cpu._params_changed()
    return gpu, cpu


def _padded(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOC, (len(LENS), TP), generator=g), torch.randint(0, VOC, (len(LENS), STEPS), generator=g)


def test_trimmed_network_matches_fp32_cpu_rows_alone():
    """bf16 on the kernels: a 70-token padded prefill (the causal flash forward), rnnTrimState to 70 / 64 / 63 / 5
    tokens, 6 steps; against the same weights in fp32 on the CPU, every row alone and unpadded."""
    gpu, cpu = _nets()
    x, cont = _padded(0)
    rows = []
    for b, n in enumerate(LENS):
        cpu.rnnClearPreviousState()
        outs = [cpu.rnnTimeStep(x[b:b + 1, :n])[0][:, :, -1:]]
        outs += [cpu.rnnTimeStep(cont[b:b + 1, t:t + 1])[0] for t in range(STEPS)]
        rows.append(torch.cat(outs, 2))
    ref = torch.cat(rows)
    from deeplearning4j_amd.ops import fallback
    fallback.reset()
    gpu.rnnClearPreviousState()
    first = gpu.rnnTimeStep(x.to(DEV))[0]
    gpu.rnnTrimState(LENS)
    outs = [torch.stack([first[b, :, n - 1] for b, n in enumerate(LENS)])[:, :, None]]
    cd = cont.to(DEV)
    outs += [gpu.rnnTimeStep(cd[:, t:t + 1])[0] for t in range(STEPS)]
    got = torch.cat(outs, 2).cpu()
    torch.cuda.synchronize()
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    assert torch.isfinite(got).all()
    for b in range(len(LENS)):
        print(f"row {b} ({LENS[b]} tokens): rel {(got[b] - ref[b]).norm() / ref[b].norm():.3e}")
    rel = (got - ref).norm() / ref.norm()
    print(f"trimmed rnnTimeStep bf16 GPU vs fp32 CPU rows alone: rel {rel:.3e}")
    assert rel < 3e-2, rel
    assert max((got[b] - ref[b]).norm() / ref[b].norm() for b in range(len(LENS))) < 3e-2
    st = gpu.rnnGetPreviousState("enc1")
    assert st["kv"].shape == (4, TP + STEPS, 256)
    assert torch.equal(st["short"].cpu(), torch.tensor([TP - n for n in LENS], dtype=torch.int32))
    gpu.rnnClearPreviousState()


@pytest.mark.parametrize("kw", [dict(), dict(numBeams=3)], ids=["greedy", "beam"])
def test_generate_does_not_see_the_padding(kw):
    gpu, _ = _nets()
    x, _ = _padded(1)
    other = x.clone()
    for b, n in enumerate(LENS):
        other[b, n:] = (other[b, n:] + 4) % VOC
    from deeplearning4j_amd.ops import fallback
    fallback.reset()
    a = gpu.generate(x.to(DEV), promptLengths=LENS, maxNewTokens=8, **kw)
    b = gpu.generate(other.to(DEV), promptLengths=LENS, maxNewTokens=8, **kw)
    assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.scores, b.scores) and torch.equal(a.lengths, b.lengths)
    assert torch.isfinite(a.scores).all()
    # the full-length row does not depend on the rows next to it: the same tokens as the row alone
    one = gpu.generate(x[:1].to(DEV), maxNewTokens=8, **kw)
    assert torch.equal(one.tokens, a.tokens[:1])


def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


_ALLOWED = ("bfloat16tofloat32_copy_kernel",)       # rnnTimeStep's fp32 copy of the output, as in the existing audit


def test_trimmed_decode_step_launches_no_torch_compute_kernels():
    from torch.profiler import ProfilerActivity, profile
    from deeplearning4j_amd.models import TextGenerationTransformer
    net = TextGenerationTransformer(numLabels=77, inputShape=[64], hidden=128, layers=2, heads=2, maxPositions=64,
                                    dataType=DataType.BFLOAT16).init(device=DEV)
    x = torch.randint(0, 77, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    steps = [x[:, t:t + 1].contiguous() for t in range(3)]
    net.rnnClearPreviousState()
    net.rnnTimeStep(x)
    net.rnnTrimState([8, 3, 1, 6])
    net.rnnTimeStep(steps[0])                                  # warm-up: kernel choices, cache allocation
    net.rnnTimeStep(steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 10, names
    for n in names:
        print("  kernel:", n[:120])
    assert sum("attn_decode_ragged_kernel" in n for n in names) == 2
    assert sum("attn_kv_append_ragged_kernel" in n for n in names) == 2
    assert sum("bert_embed_fwd_ragged_kernel" in n for n in names) == 1
    assert not any("attn_decode_kernel" in n for n in names)
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a trimmed decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks
