"""The generation kernels of csrc/generation.hip (row sampler, beam step, cache gather) against the fp64 host oracles
of ops/generation_native.py, rnnReorderState on the kernels, and generate() end to end on the GPU."""
import pytest
import torch

from deeplearning4j_amd import *  # noqa: F401,F403
from deeplearning4j_amd.models import TextGenerationTransformer, TransformerSeq2Seq
from deeplearning4j_amd.ops import fallback
from deeplearning4j_amd.ops import generation_native as GN
from deeplearning4j_amd.ops.nn_misc import PhiloxStream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SETTINGS = ((0, 1.0, 1.0), (2, 1.0, 1.0), (0, 0.9, 0.7), (5, 0.5, 1.3))        # (topK, topP, temperature)


def _rng(seed, offset=0):
    s = PhiloxStream(DEV)
    s.seed = seed
    s.offset.fill_(offset)
    return s


def sampler_rows(R, V, dtname):
    """Probabilities [R, V] as stored in ``dtname`` (made on the CPU, so the same everywhere). The generator seed is
    chosen per shape so that no row sits on a top-p boundary (checked by ``boundary_margin_ok`` inside the test)."""
    seed = 100 * V + 10 * R + list(DTYPES).index(dtname) + _SEED_SHIFT.get((R, V, dtname), 0)
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(R, V, generator=g), 1).to(DTYPES[dtname])


# The required distance from a top-p boundary is 1e-5 * keptMass; every default seed has it, and the shapes that were
# within 1e-4 got another seed (searched on the CPU) that leaves more than ten times the requirement.
_SEED_SHIFT = {(3, 1000, "fp32"): 1001, (3, 1000, "bf16"): 1000, (3, 4099, "fp32"): 1040, (3, 4099, "bf16"): 1006,
               (3, 4099, "fp16"): 1007}


def boundary_margin_ok(p, topK, topP, temp):
    keep, w, margin = GN.sample_kept_set(p, temp, topK, topP)
    kept = (w * keep).sum(1)
    return bool((margin >= 1e-5 * kept).all())


# ------------------------------------------------------------------------------------------------ 8: sampler
@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("V", [1, 5, 77, 1000, 4099])
def test_sampler_against_the_fp64_oracle(V, dtname):
    for R in (1, 3):
        p = sampler_rows(R, V, dtname)
        pd = p.to(DEV)
        for si, (topK, topP, temp) in enumerate(SETTINGS):
            assert boundary_margin_ok(p, topK, topP, temp), "test input on a top-p boundary: pick another seed"
            seed, off = 1234 + si, 3 + si
            rng = _rng(seed, off)
            tok, logp, u = GN.sample_rows_native(pd, temp, topK, topP, False, rng, want_u=True)
            tok2, logp2, u2 = GN.sample_rows_native(pd, temp, topK, topP, False, rng, want_u=True)
            assert torch.equal(tok, tok2) and torch.equal(logp, logp2) and torch.equal(u, u2)   # bitwise, run to run
            tok, logp, u = tok.cpu(), logp.cpu(), u.cpu()
            assert tok.dtype == torch.int64
            assert torch.equal(u, GN.sample_uniform(seed, off, R))
            keep, w, _ = GN.sample_kept_set(p, temp, topK, topP)
            cdf = torch.cumsum(w * keep, 1)
            for r in range(R):
                t = int(tok[r])
                kept = float(cdf[r, -1])
                target, eps = float(u[r]) * kept, 1e-5 * kept
                lo = float(cdf[r, t - 1]) if t > 0 else 0.0
                print(f"V={V} {dtname} R={R} set={si} row={r}: tok={t} target={target:.9g} "
                      f"cdf=[{lo:.9g}, {float(cdf[r, t]):.9g}] kept={kept:.6g}")
                assert bool(keep[r, t]), (r, t)
                assert lo - eps <= target <= float(cdf[r, t]) + eps
                want = float(torch.log(p[r, t].double()))
                assert abs(float(logp[r]) - want) <= 1e-6 * max(abs(want), 1e-30) + 1e-12, (float(logp[r]), want)


def _tie_rows(V=8):
    g = torch.Generator().manual_seed(12)
    rand = torch.softmax(2.0 * torch.randn(V, generator=g), 0)
    tied = rand.clone()
    tied[3] = tied[5] = tied.max()
    tied = tied / tied.sum()
    onehot = torch.zeros(V)
    onehot[6] = 1.0
    return {"tiedmax": tied, "equal": torch.full((V,), 1.0 / V), "onehot": onehot}


@pytest.mark.parametrize("dtname", list(DTYPES))
def test_sampler_ties_and_zeros(dtname):
    for name, row in _tie_rows().items():
        p = row.to(DTYPES[dtname]).reshape(1, 8).repeat(256, 1)
        for topK, topP in ((0, 1.0), (1, 1.0), (2, 1.0), (8, 1.0), (11, 1.0), (0, 0.9), (0, 1e-6), (2, 0.9)):
            keep = GN.sample_kept_set(p[:1], 1.0, topK, topP)[0][0]
            tok = GN.sample_rows_native(p.to(DEV), 1.0, topK, topP, False, _rng(77))[0].cpu()
            drawn = torch.zeros(8, dtype=torch.bool)
            drawn[tok] = True
            assert not (drawn & ~keep).any(), (name, topK, topP, drawn, keep)
            if name == "equal":
                assert keep.all() and drawn.all()                # ties all kept; 256 draws reach all 8
            if name == "onehot":
                assert drawn.tolist() == [i == 6 for i in range(8)]
            if name == "tiedmax" and (topK == 1 or topP == 1e-6):
                assert int(keep.sum()) == 3 and torch.equal(drawn, keep)     # all tied maxima, nothing else


def test_sampler_with_more_tied_top_k_survivors_than_fit_in_lds():
    """top-k 5 of an all-equal row of 4099 keeps all 4099 (ties): more survivors than the kernel gathers into LDS, so
    it passes over the row instead; a row with 1024 tied maxima just fits."""
    flat = torch.full((64, 4099), 1.0 / 4099)
    edge = torch.full((64, 4099), 1e-4)
    edge[:, 5:4 * 1024 + 5:4] = 5e-4
    for p, nkeep in ((flat, 4099), (edge, 1024)):
        p = p.to(torch.bfloat16)
        keep, w, _ = GN.sample_kept_set(p[:1], 1.0, 5, 1.0)
        assert int(keep.sum()) == nkeep
        tok, logp, u = (t.cpu() for t in GN.sample_rows_native(p.to(DEV), 1.0, 5, 1.0, False, _rng(3), want_u=True))
        cdf = torch.cumsum(w[0] * keep[0], 0)
        kept = float(cdf[-1])
        for r in range(64):
            t = int(tok[r])
            lo = float(cdf[t - 1]) if t > 0 else 0.0
            assert bool(keep[0, t]) and lo - 1e-5 * kept <= float(u[r]) * kept <= float(cdf[t]) + 1e-5 * kept
        assert len(set(tok.tolist())) > 32


def test_sampler_greedy_finished_and_count():
    p = torch.tensor([[0.1, 0.3, 0.3, 0.3], [0.25, 0.25, 0.25, 0.25], [0.7, 0.1, 0.1, 0.1]], device=DEV)
    tok, logp, u = GN.sample_rows_native(p, greedy=True, want_u=True)
    assert tok.tolist() == [1, 0, 0] and u.tolist() == [0.0, 0.0, 0.0]
    assert torch.allclose(logp.cpu(), torch.log(torch.tensor([0.3, 0.25, 0.7])), rtol=1e-6)
    big = torch.zeros(2, 4099, device=DEV, dtype=torch.bfloat16)
    big[0, 4098] = big[0, 300] = 0.5
    big[1, 4097] = 1.0
    assert GN.sample_rows_native(big, greedy=True)[0].tolist() == [300, 4097]
    # finished rows: padToken, log-prob 0; eos marks a row; the count is of the rows still unfinished
    fin = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    tok, logp, _ = GN.sample_rows_native(p, greedy=True, finished=fin, eosToken=1, padToken=9, count=count)
    assert tok.tolist() == [1, 9, 0] and float(logp[1]) == 0.0
    assert fin.tolist() == [1, 1, 0] and int(count) == 1
    rng = _rng(5)
    tok, logp, _ = GN.sample_rows_native(p, 1.0, 0, 1.0, False, rng, finished=fin, eosToken=3, padToken=9,
                                         count=count, advance=True)
    assert tok[:2].tolist() == [9, 9] and int(rng.offset) == 1 and int(count) == (0 if int(tok[2]) == 3 else 1)
    # refused operands
    assert GN.sample_rows_native(p, 0.0, 0, 1.0, False, rng) is None
    assert GN.sample_rows_native(p, 1.0, 0, 0.0, False, rng) is None


# ------------------------------------------------------------------------------------------------ 9: beam step
@pytest.mark.parametrize("V", [3, 77, 4099])
@pytest.mark.parametrize("W", [1, 2, 3, 8, 16])
def test_beam_step_is_valid_against_the_fp64_oracle(W, V):
    eos, pad = 1, 2
    for B in (1, 3):
        for dtname in ("fp32", "bf16"):
            g = torch.Generator().manual_seed(1000 * W + V + B)
            score = torch.full((B, W), float("-inf"))
            score[:, 0] = 0.0
            fin = torch.zeros(B, W, dtype=torch.uint8)
            length = torch.zeros(B, W, dtype=torch.int32)
            ds, df, dl = score.to(DEV), fin.to(DEV), length.to(DEV)
            count = torch.zeros(1, dtype=torch.int32, device=DEV)
            for step in range(4):
                p = torch.softmax(2.0 * torch.randn(B * W, V, generator=g), 1).to(DTYPES[dtname])
                if step == 0:
                    p[0, 0] = 0.0                                # log 0 = -inf among the candidates
                s0, f0, l0 = ds.cpu(), df.cpu(), dl.cpu()
                par, tok = GN.beam_step_native(p.to(DEV), ds, df, dl, eos, pad, count)
                par, tok, s1, f1, l1 = par.cpu(), tok.cpu(), ds.cpu(), df.cpu(), dl.cpu()
                want = GN.beam_step_reference(p, s0, f0, l0, eos, pad)
                x = p.double().reshape(B, W, V)
                for b in range(B):
                    w = par[b] - b * W
                    assert ((w >= 0) & (w < W)).all()
                    flat = w.long() * V + torch.where(f0[b][w.long()] != 0, torch.full_like(tok[b], pad), tok[b])
                    assert len(set(flat.tolist())) == W, "candidates not distinct"
                    assert (s1[b][:-1] >= s1[b][1:]).all(), "not sorted by score"
                    for j in range(W):
                        wj, tj = int(w[j]), int(tok[b, j])
                        if f0[b, wj]:
                            exact = float(s0[b, wj])
                            assert tj == pad and int(l1[b, j]) == int(l0[b, wj]) and int(f1[b, j]) == 1
                            assert float(s1[b, j]) == exact      # finished: score unchanged
                        else:
                            exact = float(s0[b, wj].double() + torch.log(x[b, wj, tj]))
                            assert int(l1[b, j]) == int(l0[b, wj]) + 1 and int(f1[b, j]) == int(tj == eos)
                        got = float(s1[b, j])
                        if exact == float("-inf"):
                            assert got == exact
                        else:
                            assert abs(got - exact) <= 2e-5, (got, exact)
                        assert got >= float(want[2][b, W - 1]) - 2e-5        # no worse than the oracle's W-th best
                assert int(count) == int((f1 == 0).sum())


@pytest.mark.parametrize("W", [1, 3, 16])
def test_beam_step_exact_cases(W):
    B, V = 2, 77
    p = torch.full((B * W, V), 1.0 / V, device=DEV)
    score = torch.zeros(B, W, device=DEV)
    fin = torch.zeros(B, W, dtype=torch.uint8, device=DEV)
    length = torch.full((B, W), 4, dtype=torch.int32, device=DEV)
    par, tok = GN.beam_step_native(p, score, fin, length, -1, 0)
    # all candidates equal: the W lowest flat indices, i.e. beam 0 with tokens 0 .. W-1
    assert par.tolist() == [[b * W] * W for b in range(B)] and tok.tolist() == [list(range(W))] * B
    assert (length == 5).all() and (fin == 0).all()
    # two runs are bitwise equal; finished beams propagate
    g = torch.Generator().manual_seed(W)
    p = torch.softmax(torch.randn(B * W, V, generator=g), 1).to(DEV)
    outs = []
    for _ in range(2):
        score = (-torch.arange(B * W, dtype=torch.float32).reshape(B, W) * 0.37).to(DEV)
        fin = torch.zeros(B, W, dtype=torch.uint8, device=DEV)
        fin[:, 0] = 1
        length = torch.arange(B * W, dtype=torch.int32).reshape(B, W).to(DEV) + 2
        s0 = score.clone()
        par, tok = GN.beam_step_native(p, score, fin, length, 5, 9)
        outs.append((par, tok, score, fin, length))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    par, tok, score, fin, length = outs[0]
    for b in range(B):
        j = par[b].tolist().index(b * W)                         # beam 0 (score 0 / -0.37*W: the best) survives
        assert j == 0 and int(tok[b, 0]) == 9 and int(fin[b, 0]) == 1
        assert int(length[b, 0]) == b * W + 2 and float(score[b, 0]) == float(s0[b, 0])
    assert GN.beam_step_native(p.reshape(B, W * V), torch.zeros(B, 17, device=DEV),
                               torch.zeros(B, 17, dtype=torch.uint8, device=DEV),
                               torch.zeros(B, 17, dtype=torch.int32, device=DEV)) is None


def test_beam_backtrack_follows_the_parents():
    B, W, N = 3, 4, 7
    g = torch.Generator().manual_seed(0)
    toks = torch.randint(0, 50, (N, B * W), generator=g)
    parents = (torch.randint(0, W, (N, B * W), generator=g) + (torch.arange(B * W) // W * W)).to(torch.int32)
    best = torch.tensor([2, 0, 3])
    want = torch.empty(B, N, dtype=torch.int64)
    r = torch.arange(B) * W + best
    for t in range(N - 1, -1, -1):
        want[:, t] = toks[t][r]
        r = parents[t][r].long()
    fallback.reset()
    got = GN.beam_backtrack(toks.to(DEV), parents.to(DEV), best.to(DEV), W)
    assert fallback.count() == 0 and torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ 10: gather
@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
@pytest.mark.parametrize("HD", [(2, 64), (1, 128)])
@pytest.mark.parametrize("L", [1, 63, 64, 65])
def test_cache_gather(L, HD, dtname):
    Tcap, C, dt = 128, 2 * HD[0] * HD[1], DTYPES[dtname]
    g = torch.Generator().manual_seed(L)
    for mbS, parent in ((2, [1, 0]), (3, [2, 2, 0]), (2, [0, 0, 0, 1, 1, 1])):
        src = torch.randn(mbS, Tcap, C, generator=g).to(dt).to(DEV)
        keep = src.clone()
        dst = torch.full((len(parent), Tcap, C), 7.0, dtype=dt, device=DEV)
        par = torch.tensor(parent, dtype=torch.int32, device=DEV)
        assert GN.cache_gather_native(src, dst, par, L) is dst
        assert torch.equal(dst[:, :L], src[parent][:, :L])
        assert (dst[:, L:] == 7.0).all() and torch.equal(src, keep)


def test_cache_gather_refuses():
    src = torch.zeros(2, 128, 256, dtype=torch.bfloat16, device=DEV)
    dst = torch.ones(2, 128, 256, dtype=torch.bfloat16, device=DEV)
    par = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    assert GN.cache_gather_native(src, src, par, 4) is None                       # in place
    assert GN.cache_gather_native(src, dst, par, 129) is None                     # beyond the capacity
    assert GN.cache_gather_native(src, dst, par.long(), 4) is None                # parent not int32
    odd_s, odd_d = (torch.zeros(2, 128, 12, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    assert GN.cache_gather_native(odd_s, odd_d, par, 4) is None                   # C not a multiple of 8 elements
    flat = torch.zeros(2 * 128 * 256 + 8, dtype=torch.bfloat16, device=DEV)
    mis = flat[1:1 + 2 * 128 * 256].view(2, 128, 256)                             # 2 bytes off a 16-byte boundary
    assert GN.cache_gather_native(mis, dst, par, 4) is None
    assert GN.cache_gather_native(src, mis, par, 4) is None
    assert (dst == 1).all()


# ------------------------------------------------------------------------------------------------ 11: layers
def _lm(dt, device, V=11):
    return TextGenerationTransformer(numLabels=V, hidden=128, layers=2, heads=2, inputShape=[16], maxPositions=96,
                                     seed=5, dataType=dt).init(device=device)


def _s2s(dt, device, V=11):
    return TransformerSeq2Seq(numLabels=V, hidden=128, layers=2, heads=2, inputShape=[8, 16], maxPositions=96,
                              seed=6, dataType=dt).init(device=device)


def _copy_params(dst, src):
    with torch.no_grad():
        dst.flattenedParams.copy_(src.flattenedParams.to(dst.flattenedParams.device))
    dst._params_changed()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


def test_reorder_state_on_the_kernels_matches_fp32_cpu():
    """The reorder case of tests/test_generation.py on the bf16 kernels against the fp32 CPU run, compared as
    tests/test_gpu_attention_decode.py compares its layers (relative L2 error below 3e-2)."""
    g = torch.Generator().manual_seed(1)
    a, b = torch.randint(0, 11, (3, 5), generator=g), torch.randint(0, 11, (4, 1), generator=g)
    parents = [2, 0, 0, 1]
    gpu, cpu = _lm(DataType.BFLOAT16, DEV), _lm(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    cpu.rnnClearPreviousState()
    cpu.rnnTimeStep(a[parents])
    want = cpu.rnnTimeStep(b)[0]
    fallback.reset()
    gpu.rnnClearPreviousState()
    gpu.rnnTimeStep(a.to(DEV))
    gpu.rnnReorderState(torch.tensor(parents, dtype=torch.int32, device=DEV))
    got = gpu.rnnTimeStep(b.to(DEV))[0]
    assert fallback.count() == 0, fallback.summary()
    assert _rel(got, want) < 3e-2
    # steady state: the two buffers swap, nothing is allocated
    enc = gpu.layers_by_name["decoder_0"]
    perm = torch.tensor([1, 0, 3, 2], dtype=torch.int32, device=DEV)
    gpu.rnnReorderState(perm)
    p0, p1 = enc._kv.data_ptr(), enc._kv_alt.data_ptr()
    gpu.rnnReorderState(perm)
    assert (enc._kv.data_ptr(), enc._kv_alt.data_ptr()) == (p1, p0)
    assert fallback.count() == 0, fallback.summary()


@pytest.mark.parametrize("grouped", [False, True])
def test_reorder_state_seq2seq_on_the_kernels(grouped):
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 11, (2, 6), generator=g)
    smask = torch.tensor([[1., 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]])
    start = torch.randint(0, 11, (2, 3), generator=g)
    t1, t2 = torch.randint(0, 11, (4, 1), generator=g), torch.randint(0, 11, (4, 1), generator=g)
    expand, perm = torch.tensor([0, 0, 1, 1]), torch.tensor([1, 0, 3, 3])
    gpu, cpu = _s2s(DataType.BFLOAT16, DEV), _s2s(DataType.FLOAT, CPU)
    _copy_params(cpu, gpu)
    rows = expand[perm]
    cpu.rnnClearPreviousState()
    cpu.rnnTimeStep(src[rows], start[rows], masks=[smask[rows], None])
    cpu.rnnTimeStep(None, t1[perm])
    want = cpu.rnnTimeStep(None, t2)[0]
    fallback.reset()
    gpu.rnnClearPreviousState()
    gpu.rnnTimeStep(src.to(DEV), start.to(DEV), masks=[smask.to(DEV), None])
    gpu.rnnReorderState(expand.int().to(DEV))
    gpu.rnnTimeStep(None, t1.to(DEV))
    gpu.rnnReorderState(perm.int().to(DEV), groupSize=2 if grouped else None)
    got = gpu.rnnTimeStep(None, t2.to(DEV))[0]
    assert fallback.count() == 0, fallback.summary()
    assert _rel(got, want) < 3e-2


# ------------------------------------------------------------------------------------------------ 12: end to end
def _loop_greedy(net, first, n, V):
    """The loop a user writes on rnnTimeStep: argmax of the fp32 output, fed back."""
    net.rnnClearPreviousState()
    out = net.rnnTimeStep(*first[0], **first[1])[0]
    toks, logp = [], torch.zeros(out.shape[0], dtype=torch.float64)
    for _ in range(n):
        p = out[:, :, -1]
        t = p.argmax(1)
        logp += torch.log(p.double().gather(1, t[:, None]))[:, 0].cpu()
        toks.append(t)
        out = net.rnnTimeStep(*([None] * (len(first[0]) - 1) + [t[:, None]]))[0]
    return torch.stack(toks, 1).cpu(), logp


def test_generate_end_to_end_transformer():
    V, N = 77, 12
    net = _lm(DataType.BFLOAT16, DEV, V)
    prompt = torch.randint(0, V, (3, 5), generator=torch.Generator().manual_seed(2)).to(DEV)
    want, logp = _loop_greedy(net, ((prompt,), {}), N, V)
    fallback.reset()
    r = net.generate(prompt, maxNewTokens=N, lengthPenalty=0.0)
    assert torch.equal(r.tokens.cpu(), want)
    assert (r.scores.cpu().double() - logp).abs().max() < 2e-5 * N
    b = net.generate(prompt, maxNewTokens=N, numBeams=4, lengthPenalty=0.0)
    print("greedy", r.scores.tolist(), "beam4", b.scores.tolist())
    assert (b.scores >= r.scores - 2e-5 * N).all()
    s1 = net.generate(prompt, maxNewTokens=N, doSample=True, topK=20, topP=0.95, temperature=0.8, seed=4)
    s2 = net.generate(prompt, maxNewTokens=N, doSample=True, topK=20, topP=0.95, temperature=0.8, seed=4)
    assert torch.equal(s1.tokens, s2.tokens) and torch.equal(s1.scores, s2.scores)
    assert fallback.count() == 0, fallback.summary()
    eos = int(want[0, 3])
    e = [net.generate(prompt, maxNewTokens=N, eosToken=eos, padToken=V - 1, eosCheckEvery=k) for k in (1, 1000)]
    assert torch.equal(e[0].tokens, e[1].tokens) and int(e[0].lengths[0]) <= 4
    assert (e[0].tokens[0, int(e[0].lengths[0]):] == V - 1).all()


def test_generate_end_to_end_seq2seq():
    V, N = 11, 8
    net = _s2s(DataType.BFLOAT16, DEV, V)
    g = torch.Generator().manual_seed(4)
    src = torch.randint(0, V, (2, 6), generator=g).to(DEV)
    smask = torch.tensor([[1., 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1]], device=DEV)
    start = torch.ones(2, 1, dtype=torch.int64, device=DEV)
    want, logp = _loop_greedy(net, ((src, start), dict(masks=[smask, None])), N, V)
    fallback.reset()
    r = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=N, lengthPenalty=0.0)
    assert torch.equal(r.tokens.cpu(), want)
    b = TransformerSeq2Seq.generate(net, src, start, sourceMask=smask, maxNewTokens=N, numBeams=4, lengthPenalty=0.0)
    assert (b.scores >= r.scores - 2e-5 * N).all()
    assert fallback.count() == 0, fallback.summary()


# ------------------------------------------------------------------------------------------------ 13: launch audit
def _is_torch_kernel(name):
    return "at::native" in name or "at6native" in name or name.startswith("void at::") or "elementwise_kernel" in name


def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("mode", ["greedy", "sample", "beam2"])
def test_generation_steps_launch_no_torch_compute_kernels(mode):
    """A steady-state step of generate() launches no torch compute kernel beyond those of a bare rnnTimeStep step,
    which ends in the fp32 conversion generate() skips: so none at all. Measured as the difference between two calls
    that differ only in the number of steps (set-up and the final gather of the result are the same in both), and
    with eosToken=None there is no device-to-host copy in the whole call."""
    kw = {"greedy": {}, "sample": dict(doSample=True, topK=10, topP=0.9, seed=1), "beam2": dict(numBeams=2)}[mode]
    net = _lm(DataType.BFLOAT16, DEV, 77)
    prompt = torch.randint(0, 77, (4, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    net.generate(prompt, maxNewTokens=6, **kw)                   # warm-up: kernel choices, allocations
    short = _profile(lambda: net.generate(prompt, maxNewTokens=4, **kw))
    long = _profile(lambda: net.generate(prompt, maxNewTokens=7, **kw))
    for names in (short, long):
        assert not [n for n in names if "DtoH" in n or "Device -> Host" in n], "device-to-host copy without an eos"
    ours = "gen_beam_kernel" if mode == "beam2" else "gen_sample_kernel"
    assert sum(ours in n for n in long) - sum(ours in n for n in short) == 3
    assert sum("attn_decode_kernel" in n for n in long) - sum("attn_decode_kernel" in n for n in short) == 6
    if mode == "beam2":
        assert sum("gen_gather_kernel" in n for n in long) - sum("gen_gather_kernel" in n for n in short) == 6
    ts, tl = ([n for n in names if _is_torch_kernel(n)] for names in (short, long))
    for n in sorted(set(tl)):
        print("  torch:", tl.count(n), ts.count(n), n[:140])
    assert len(tl) == len(ts), f"torch compute kernels grow with the number of steps: {len(ts)} -> {len(tl)}"
