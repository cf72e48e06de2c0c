"""The fp8 key/value cache on the GPU (csrc/attention_decode.hip): the quantising append against the torch reference
bit for bit, the fp8 decode attention bitwise against the 16-bit kernel on the dequantised cache (uniform and per-row
positions, every split count), refusals, and the layers / generate() on top of them. Shapes, positions, error measure
and bounds: tests/test_gpu_attention_decode.py and tests/test_gpu_ragged_decode.py."""
import functools

import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import transformer_native as TN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
SHAPES = [(2, 2, 64), (1, 3, 128)]
POS_TN = [(0, 1), (62, 1), (63, 1), (64, 1), (128, 1), (60, 3), (50, 17), (10, 65), (191, 2)]
DTYPES = [torch.bfloat16, torch.float16]
NAN8 = 0x7F                                  # the e4m3fn NaN: a byte of an unwritten row that reaches a product shows


def _err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


@functools.lru_cache(maxsize=None)
def _seq(dt, B, H, D, L, seed=0):
    """qkv [B, L, 3E] in dt on the CPU (randn * 0.8) and the fp8 rows of its K | V columns by the reference
    quantisation [B, L, R]. Computed once per case and never modified."""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + D + 7 * L + seed * 7919)
    qkv = (torch.randn(B, L, 3 * H * D, generator=g) * 0.8).to(dt)
    return qkv, TN.kv_fp8_quantize_reference(qkv[:, :, H * D:], H)


def _tcap(L):
    return (L // 64 + 1) * 64 + 64


def _rows(H, D):
    return TN.kv_fp8_row_bytes(H, D)


# ------------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("pos,Tn", POS_TN)
@pytest.mark.parametrize("B,H,D", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_append_is_the_reference_quantisation(dt, B, H, D, pos, Tn):
    qkv, want = _seq(dt, B, H, D, pos + Tn)
    new = qkv[:, pos:].to(DEV).contiguous()
    g = torch.Generator().manual_seed(pos + Tn)
    before = torch.randint(0, 256, (B, _tcap(pos + Tn), _rows(H, D)), generator=g, dtype=torch.uint8).to(DEV)
    kv = before.clone()
    assert TN.attn_decode_supported(new, kv, H)
    assert TN.attn_kv_append(new, kv, H, pos) is kv
    assert torch.equal(kv[:, pos:pos + Tn].cpu(), want[:, pos:]), "codes, scale bytes or zero pad differ"
    assert torch.equal(kv[:, :pos], before[:, :pos]) and torch.equal(kv[:, pos + Tn:], before[:, pos + Tn:])


@pytest.mark.parametrize("dt", DTYPES)
def test_append_special_groups_and_the_capacity(dt):
    B, H, D, Tcap, Tn = 2, 3, 64, 128, 5
    E = H * D
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Tn, 3 * E, generator=g) * 0.8
    x[0, 0, E:E + D] = 0.0                                         # an all-zero group
    x[0, 1, E + D:E + 2 * D] *= 2.0 ** -10
    x[1, 2, 3 * E - D:] *= 2.0 ** 6
    qkv = x.to(dt)
    want = TN.kv_fp8_quantize_reference(qkv[:, :, E:], H)
    new = qkv.to(DEV)
    before = torch.full((B, Tcap, _rows(H, D)), NAN8, dtype=torch.uint8, device=DEV)
    kv = before.clone()
    assert TN.attn_kv_append(new, kv, H, Tcap - Tn + 1) is None             # pos + Tn > Tcap: status -1
    assert torch.equal(kv, before)
    assert TN.attn_kv_append(new, kv, H, Tcap - Tn) is kv                   # the last rows of the cache
    assert torch.equal(kv[:, Tcap - Tn:].cpu(), want) and torch.equal(kv[:, :Tcap - Tn], before[:, :Tcap - Tn])
    assert kv[0, Tcap - Tn, 2 * E] == 127                                   # the all-zero group's scale byte


@pytest.mark.parametrize("Tn", [1, 3])
@pytest.mark.parametrize("H,D", [(2, 64), (3, 128)])
@pytest.mark.parametrize("dt", DTYPES)
def test_ragged_append(dt, H, D, Tn):
    """Shortfalls 0, in between, pos itself, and values outside [0, pos] (clamped): every row's new bytes are the
    reference's at its own position and nothing else changes."""
    pos, shorts = 70, (0, 7, 70, -3, 1000)
    B = len(shorts)
    qkv, want = _seq(dt, B, H, D, Tn, seed=1)
    new = qkv.to(DEV)
    g = torch.Generator().manual_seed(9)
    before = torch.randint(0, 256, (B, 128, _rows(H, D)), generator=g, dtype=torch.uint8).to(DEV)
    kv = before.clone()
    short = torch.tensor(shorts, dtype=torch.int32, device=DEV)
    assert TN.attn_kv_append(new, kv, H, pos, short=short) is kv
    for b, s in enumerate(shorts):
        p = pos - min(max(s, 0), pos)
        assert torch.equal(kv[b, p:p + Tn].cpu(), want[b]), f"row {b}: the new rows are not at {p}"
        assert torch.equal(kv[b, :p], before[b, :p]) and torch.equal(kv[b, p + Tn:], before[b, p + Tn:])
    assert TN.attn_kv_append(new, kv, H, pos, short=short.long()) is None


# ------------------------------------------------------------------------------------------------ decode
def _caches(dt, B, H, D, poss, Tn):
    """Row b holds its own sequence of poss[b] + Tn tokens. -> (new chunk [B, Tn, 3E], the fp8 cache prefilled with
    the NaN byte and written by the append kernel (history, then the chunk), the NaN-filled 16-bit cache holding the
    dequantised valid rows, shortfall against max(poss) or None for equal positions, fp32 oracles per row on the
    dequantised values)."""
    pos, E = max(poss), H * D
    tcap = _tcap(pos + Tn)
    kv8 = torch.full((B, tcap, _rows(H, D)), NAN8, dtype=torch.uint8, device=DEV)
    kv16 = torch.full((B, tcap, 2 * E), float("nan"), dtype=dt, device=DEV)
    uniform = len(set(poss)) == 1
    seqs = [_seq(dt, B, H, D, pos + Tn)[0]] * B if uniform else [_seq(dt, 1, H, D, p + Tn, seed=b)[0]
                                                                  for b, p in enumerate(poss)]
    news, refs = [], []
    for b, p in enumerate(poss):
        q = (seqs[b][b:b + 1] if uniform else seqs[b]).to(DEV)
        h1 = p // 2
        for lo, hi in ((0, h1), (h1, p)):
            if hi > lo:
                assert TN.attn_kv_append(q[:, lo:hi].contiguous(), kv8[b:b + 1], H, lo) is not None
        news.append(q[:, p:])
    new = torch.cat(news).contiguous()
    short = None if uniform else torch.tensor([pos - p for p in poss], dtype=torch.int32, device=DEV)
    assert TN.attn_kv_append(new, kv8, H, pos, short=short) is kv8
    for b, p in enumerate(poss):
        L = p + Tn
        assert (kv8[b, L:] == NAN8).all(), f"row {b}: the append wrote past {L}"
        deq = TN.kv_fp8_dequantize_reference(kv8[b:b + 1, :L].cpu(), H, D, torch.float32)
        assert torch.equal(deq.to(dt).float(), deq), "a dequantised value is not exact in the 16-bit dtype"
        kv16[b, :L] = deq[0].to(dt).to(DEV)
        refs.append(TN.attention_decode_reference(new[b:b + 1, :, :E].float().cpu(), deq[:, :, :E], deq[:, :, E:], H, p))
    return new, kv8, kv16, short, torch.cat(refs)


@pytest.mark.parametrize("pos,Tn", POS_TN)
@pytest.mark.parametrize("B,H,D", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_is_the_16_bit_kernel_on_the_dequantised_cache(dt, B, H, D, pos, Tn):
    new, kv8, kv16, _, ref = _caches(dt, B, H, D, (pos,) * B, Tn)
    out = TN.attn_decode(new, kv8, H, pos)
    assert out is not None and out.dtype == dt and out.shape == (B, Tn, H * D)
    assert torch.isfinite(out).all(), "a row past the valid length reached the products"
    assert torch.equal(out, TN.attn_decode(new, kv16, H, pos)), "not the 16-bit kernel's bits"
    e = _err(out, ref)
    print(f"fp8 decode {dt} B={B} H={H} D={D} pos={pos} Tn={Tn}: err {e:.3e}")
    assert e < 2e-2


@pytest.mark.parametrize("Tn", [1, 17])
@pytest.mark.parametrize("B,H,D", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_splits(dt, B, H, D, Tn):
    pos = 300
    new, kv8, kv16, _, ref = _caches(dt, B, H, D, (pos,) * B, Tn)
    for splits in (1, 2, 3, 5, 64):
        a = TN.attn_decode(new, kv8, H, pos, splits=splits)
        assert torch.isfinite(a).all()
        assert torch.equal(a, TN.attn_decode(new, kv8, H, pos, splits=splits)), f"splits={splits} is not reproducible"
        assert torch.equal(a, TN.attn_decode(new, kv16, H, pos, splits=splits)), f"splits={splits}: not the 16-bit bits"
        e = _err(a, ref)
        print(f"fp8 splits={splits} {dt} B={B} H={H} D={D} Tn={Tn}: err {e:.3e}")
        assert e < 2e-2


@pytest.mark.parametrize("H,D", [(2, 64), (3, 128)])
@pytest.mark.parametrize("dt", DTYPES)
def test_ragged_decode_splits(dt, H, D):
    """Upper bound 300 keys, rows of 300 / 257 / 70 / 1 keys, one new query per row."""
    Tn, lens = 1, (300, 257, 70, 1)
    poss = tuple(n - Tn for n in lens)
    pos = max(poss)
    new, kv8, kv16, short, ref = _caches(dt, len(lens), H, D, poss, Tn)
    for splits in (1, 2, 3, 5, 64):
        a = TN.attn_decode(new, kv8, H, pos, splits=splits, short=short)
        assert torch.isfinite(a).all(), "a row past a batch row's own length reached the products"
        assert torch.equal(a, TN.attn_decode(new, kv8, H, pos, splits=splits, short=short))
        assert torch.equal(a, TN.attn_decode(new, kv16, H, pos, splits=splits, short=short)), \
            f"splits={splits}: not the 16-bit ragged kernel's bits"
        e = _err(a, ref)
        print(f"fp8 ragged splits={splits} {dt} H={H} D={D}: err {e:.3e}")
        assert e < 2e-2


@pytest.mark.parametrize("Tn,poss", [(3, (60, 50, 10)), (17, (60, 50, 10)), (65, (60, 50, 10)), (1, (191, 63, 64))])
@pytest.mark.parametrize("dt", DTYPES)
def test_ragged_decode_chunks(dt, Tn, poss):
    H, D = 3, 128
    new, kv8, kv16, short, ref = _caches(dt, len(poss), H, D, poss, Tn)
    a = TN.attn_decode(new, kv8, H, max(poss), short=short)
    assert torch.isfinite(a).all()
    assert torch.equal(a, TN.attn_decode(new, kv16, H, max(poss), short=short))
    assert _err(a, ref) < 2e-2


def test_unsupported_operands_are_refused():
    B, H, Tn = 2, 2, 3
    for D, dt in ((32, torch.bfloat16), (64, torch.float32)):
        E = H * D
        qkv = torch.randn(B, Tn, 3 * E, device=DEV).to(dt)
        kv = torch.zeros(B, 64, _rows(H, D), device=DEV, dtype=torch.uint8)
        assert not TN.attn_decode_supported(qkv, kv, H)
        assert TN.attn_kv_append(qkv, kv, H, 0) is None
        assert TN.attn_decode(qkv, kv, H, 0) is None
        assert torch.count_nonzero(kv) == 0
    qkv = torch.randn(B, Tn, 3 * 128, device=DEV).to(torch.bfloat16)
    assert not TN.attn_decode_supported(qkv, torch.zeros(B, 64, 2 * 128, device=DEV, dtype=torch.uint8), H)   # not R wide
    assert not TN.attn_decode_supported(qkv, torch.zeros(B, 60, _rows(H, 64), device=DEV, dtype=torch.uint8), H)


# ------------------------------------------------------------------------------------------------ network
def _lm_graph(dt, device, T, cache=None, V=11, E=128, H=2, F=24):
    """The two-block causal language model of tests/test_gpu_attention_decode.py, with the cache format."""
    g = (NeuralNetConfiguration.Builder().seed(7).dataType(dt).updater(NoOp())
         .weightInit(NormalDistribution(0.0, 0.05)).graphBuilder())
    g.addInputs("tokens")
    g.addLayer("emb", BertEmbeddingLayer.Builder().nIn(V).nOut(E).maxPositions(T + 2).inputLength(T).build(), "tokens")
    g.addLayer("enc0", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True)
               .cacheDataType(cache).build(), "emb")
    g.addLayer("enc1", TransformerEncoderLayer.Builder().nIn(E).nOut(E).nHeads(H).ffnSize(F).causal(True)
               .cacheDataType(cache).build(), "enc0")
    g.addLayer("out", RnnOutputLayer.Builder(LossFunction.MCXENT).activation(Activation.SOFTMAX).nIn(E).nOut(V)
               .build(), "enc1")
    g.setOutputs("out")
    net = ComputationGraph(g.build())
    net.init(device=device)
    return net


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.cpu())
    dst._params_changed()


def _run(net, x, chunks):
    net.rnnClearPreviousState()
    return torch.cat([net.rnnTimeStep(x[:, a:b])[0] for a, b in chunks], 2).cpu()


def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


_ALLOWED = ("bfloat16tofloat32_copy_kernel",)        # the network API's fp32 copy of the output, once per step


def test_network_time_step_matches_fp32_cpu_with_the_same_cache():
    """bf16 GPU against fp32 CPU, both with the fp8 cache. The two sides quantise bf16 against fp32 K / V, so single
    codes can differ: the bound is the project's 3e-2 for this comparison with a 16-bit cache plus rel_q, the relative
    L2 distance between the fp8-cache and the plain-cache fp32 CPU outputs (what the quantisation itself moves)."""
    T, MB, V = 70, 3, 11
    gpu = _lm_graph(DataType.BFLOAT16, DEV, T, "fp8")
    cpu8 = _lm_graph(DataType.FLOAT, CPU, T, "fp8")
    cpu = _lm_graph(DataType.FLOAT, CPU, T)
    _copy_params(cpu8, gpu)
    _copy_params(cpu, gpu)
    x = torch.randint(0, V, (MB, T), generator=torch.Generator().manual_seed(0))
    plain = cpu.output(x)[0]
    for label, chunks in (("token by token", [(t, t + 1) for t in range(T)]),
                          ("66-token prompt + steps", [(0, 66)] + [(t, t + 1) for t in range(66, T)])):
        ref = _run(cpu8, x, chunks)
        rel_q = ((ref - plain).norm() / plain.norm()).item()
        fallback.reset()
        got = _run(gpu, x.to(DEV), chunks)
        torch.cuda.synchronize()
        assert gpu.helperCountFail() == 0, gpu.fallbackSummary()
        assert torch.isfinite(got).all()
        rel = ((got - ref).norm() / ref.norm()).item()
        print(f"fp8 cache, {label}: rel {rel:.3e} rel_q {rel_q:.3e} bound {3e-2 + rel_q:.3e}")
        assert rel < 3e-2 + rel_q, (rel, rel_q)
    st = gpu.rnnGetPreviousState("enc1")
    assert st["kvFormat"] == "fp8" and st["kv"].dtype == torch.uint8 and st["kv"].shape == (MB, T, _rows(2, 64))
    # one steady-state step: the fp8 append and decode kernels once per block, no torch compute kernel
    from torch.profiler import ProfilerActivity, profile
    steps = [x[:, t:t + 1].contiguous().to(DEV) for t in range(3)]
    gpu.rnnClearPreviousState()
    gpu.rnnTimeStep(steps[0])                                  # warm-up: kernel choices, cache allocation
    gpu.rnnTimeStep(steps[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        gpu.rnnTimeStep(steps[2])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert len(names) > 10, names
    assert sum("attn_decode_fp8_kernel" in n for n in names) == 2, names
    assert sum("attn_kv_append_fp8_kernel" in n for n in names) == 2, names
    assert not any("attn_decode_kernel" in n or "attn_kv_append_kernel" in n for n in names)
    torch_ks = [n for n in names if _is_torch_kernel(n)]
    extra = [n for n in torch_ks if not any(a in n for a in _ALLOWED)]
    assert not extra, f"torch compute kernels in a decode step: {sorted(set(extra))[:6]}"
    assert len(torch_ks) <= 1, torch_ks


def test_layer_off_the_kernels_takes_the_torch_path_with_the_same_quantisation():
    """SelfAttentionLayer with head size 32 (outside the kernels) and the fp8 cache: the torch path stores and reads the
    fp8 rows on the GPU, counted as a fallback; against the same weights in fp32 on the CPU with the fp8 cache."""
    def net(dt, device):
        b = (NeuralNetConfiguration.Builder().seed(11).dataType(dt).updater(NoOp())
             .weightInit(NormalDistribution(0, 0.05)).list())
        b.layer(0, SelfAttentionLayer.Builder().nIn(128).nOut(64).nHeads(2).causal(True).cacheDataType("fp8")
                .activation(Activation.IDENTITY).build())
        b.layer(1, RnnOutputLayer.Builder(LossFunction.MCXENT).nIn(64).nOut(5).activation(Activation.SOFTMAX).build())
        n = MultiLayerNetwork(b.build())
        n.init(device=device)
        return n
    gpu, cpu = net(DataType.BFLOAT16, DEV), net(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    x = torch.randn(2, 128, 5, generator=torch.Generator().manual_seed(3))
    cpu.rnnClearPreviousState()
    ref = torch.cat([cpu.rnnTimeStep(x[:, :, t:t + 1]) for t in range(5)], 2)
    fallback.reset()
    gpu.rnnClearPreviousState()
    got = torch.cat([gpu.rnnTimeStep(x[:, :, t:t + 1].to(DEV)) for t in range(5)], 2).cpu()
    assert fallback.count("attention") == 5
    st = gpu.rnnGetPreviousState(0)
    assert st["kvFormat"] == "fp8" and st["kv"].dtype == torch.uint8 and st["kv"].shape == (2, 5, _rows(2, 32))
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"head size 32, fp8 cache on the torch path: rel {rel:.3e}")
    assert rel < 3e-2, rel


# ------------------------------------------------------------------------------------------------ state, generation
VOC, HEADS, HS = 97, 2, 64
CACHED = ("decoder_0", "decoder_1")


@functools.lru_cache(maxsize=None)
def _lm():
    return TextGenerationTransformer(numLabels=VOC, hidden=HEADS * HS, layers=2, heads=HEADS, inputShape=[16],
                                     maxPositions=512, seed=5, dataType=DataType.BFLOAT16,
                                     cacheDataType="fp8").init(device=DEV)


def _prompt(mb, Tp, seed=0):
    return torch.randint(0, VOC, (mb, Tp), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _same(a, b):
    return torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.scores, b.scores)


def test_state_and_reorder():
    net, MB, T = _lm(), 3, 70
    fallback.reset()
    net.rnnClearPreviousState()
    net.rnnTimeStep(_prompt(MB, T))
    R = _rows(HEADS, HS)
    for parents in ([2, 0, 1], [1, 2, 0], [0, 0, 1, 1, 2, 2], [5, 4, 3, 2, 1, 0]):     # both buffers; growing rows
        before = {n: net.rnnGetPreviousState(n)["kv"] for n in CACHED}
        net.rnnReorderState(torch.tensor(parents, dtype=torch.int32, device=DEV))
        for n in CACHED:
            st = net.rnnGetPreviousState(n)
            assert st["kvFormat"] == "fp8" and st["kv"].dtype == torch.uint8
            assert st["kv"].shape == (len(parents), T, R)
            assert torch.equal(st["kv"], before[n].index_select(0, torch.tensor(parents, device=DEV)))
    torch.cuda.synchronize()
    assert net.helperCountFail() == 0, net.fallbackSummary()
    net.rnnClearPreviousState()


def test_generate_greedy_and_beams_run_on_the_kernels():
    net, mb, Tp, N = _lm(), 3, 5, 12
    fallback.reset()
    greedy = net.generate(_prompt(mb, Tp), maxNewTokens=N)
    again = net.generate(_prompt(mb, Tp), maxNewTokens=N)
    beams = net.generate(_prompt(mb, Tp), maxNewTokens=N, numBeams=4)
    torch.cuda.synchronize()
    assert net.helperCountFail() == 0, net.fallbackSummary()
    assert _same(greedy, again)
    for r in (greedy, beams):
        assert r.tokens.shape == (mb, N) and int(r.tokens.min()) >= 0 and int(r.tokens.max()) < VOC
        assert torch.isfinite(r.scores).all()
    assert net.rnnGetPreviousState(CACHED[0])["kvFormat"] == "fp8"


def test_seq2seq_decoder_keeps_its_memory_in_the_compute_dtype():
    from deeplearning4j_amd.models import TransformerSeq2Seq
    net = TransformerSeq2Seq(numLabels=VOC, hidden=HEADS * HS, layers=2, heads=HEADS, inputShape=[8, 16],
                             maxPositions=512, seed=6, dataType=DataType.BFLOAT16,
                             cacheDataType="fp8").init(device=DEV)
    src, start = _prompt(3, 8, 4), torch.zeros(3, 1, dtype=torch.int64, device=DEV)
    fallback.reset()
    want = TransformerSeq2Seq.generate(net, src, start, maxNewTokens=12, pinPositions=True)
    got = TransformerSeq2Seq.generate(net, src, start, maxNewTokens=12, useGraph=True)
    assert _same(got, want)
    assert net.helperCountFail() == 0, net.fallbackSummary()
    st = net.rnnGetPreviousState("decoder_0")
    assert st["kvFormat"] == "fp8" and st["kv"].dtype == torch.uint8 and st["kv"].shape[2] == _rows(HEADS, HS)
    assert all(v.dtype != torch.uint8 for k, v in st.items() if k != "kv" and torch.is_tensor(v) and v.is_floating_point())
    assert net.layers_by_name["encoder_0"].conf.cacheDataType is None


def test_pinned_equals_graph_replay():
    net, mb, Tp, N = _lm(), 3, 5, 24
    prompt = _prompt(mb, Tp)
    fallback.reset()
    pinned = net.generate(prompt, maxNewTokens=N, pinPositions=True)
    assert net.lastGenerationStats == {"captures": 0, "graphReplays": 0, "eagerSteps": N}
    kv = {n: net.rnnGetPreviousState(n)["kv"] for n in CACHED}
    got = net.generate(prompt, maxNewTokens=N, useGraph=True)
    st = net.lastGenerationStats
    assert st["captures"] == 1 and st["graphReplays"] > 0
    assert _same(got, pinned)
    real = Tp + N - 1
    for n in CACHED:
        assert torch.equal(net.rnnGetPreviousState(n)["kv"][:, :real], kv[n][:, :real])
    assert net.helperCountFail() == 0, net.fallbackSummary()


def test_ragged_prompts_equal_every_row_alone():
    """Prompt and continuation stay below 64 keys: one split at every step, and every chunk (the padded prompt as
    well as a row's own) goes through the decode kernel over the cache."""
    net, Tp, lens, N = _lm(), 40, (1, 5, 33, 40), 20
    for L in range(1, Tp + N + 1):
        assert TN.attn_decode_splits(len(lens), 1, HEADS, HS, L) == 1 == TN.attn_decode_splits(1, 1, HEADS, HS, L)
    prompt = _prompt(len(lens), Tp, 2)
    fallback.reset()
    got = net.generate(prompt, promptLengths=lens, maxNewTokens=N)
    for b, n in enumerate(lens):
        alone = net.generate(prompt[b:b + 1, :n].contiguous(), maxNewTokens=N)
        assert torch.equal(got.tokens[b:b + 1], alone.tokens), f"row {b} ({n} tokens)"
    assert net.helperCountFail() == 0, net.fallbackSummary()
