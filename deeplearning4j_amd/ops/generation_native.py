"""Token generation ops: the ctypes wrappers of csrc/generation.hip (row sampler, beam-search step, key/value-cache
row gather), a torch implementation of each with the same semantics for tensors the kernels do not take (CPU, fp64;
counted through ``ops.fallback`` on a GPU), and the host oracles the tests compare both against.

The semantics (weights, top-k / top-p thresholds with ties kept, the Philox draw, the beam total order) are written
out at the top of csrc/generation.hip. The speculative-decoding ops at the end of the file (verify, commit, n-gram
draft, keep) wrap csrc/speculative.hip in the same way."""
import torch

from . import fallback, native
from .dispatch import use_native
from .native import _check, _ptr, _stream
from .transformer_native import philox4x32_10

PHILOX_TAG = 0x47454E53
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
_NEG_INF = float("-inf")


def _kernel_ok(p):
    return use_native(p, "generation") and p.dtype in _DT and p.dim() == 2 and p.is_contiguous() and \
        p.numel() < 2 ** 31


# ------------------------------------------------------------------------------------------------ oracles (host)
def sample_uniform(seed, offset, rows):
    """The sampler's uniforms for rows 0 .. rows-1 at counter value ``offset``: fp32 [rows] in [0, 1), 24 bits of
    word 0 of philox4x32_10({row, 0, PHILOX_TAG, offset mod 2^32}, {seed low, seed high})."""
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    off = int(offset) & 0xFFFFFFFF
    return torch.tensor([(philox4x32_10((r, 0, PHILOX_TAG, off), key)[0] >> 8) / 16777216.0 for r in range(int(rows))],
                        dtype=torch.float32)


def sample_kept_set(p, temperature=1.0, topK=0, topP=1.0):
    """fp64 oracle of the sampler's kept set for probabilities p [R, V] (any float dtype; the values as stored).
    -> (keep bool [R, V], w fp64 [R, V] weights relative to the row maximum, margin fp64 [R]): ``margin`` is the
    distance of topP * M from the nearest achievable kept mass (inf when top-p is off) — a row whose margin is small
    against its kept mass sits on a top-p boundary that fp32 sums may resolve either way."""
    x = torch.nan_to_num(p.detach().cpu().to(torch.float64), nan=0.0).clamp_min(0.0)
    R, V = x.shape
    mx = x.max(dim=1, keepdim=True).values
    w = torch.where(x > 0, torch.exp((torch.log(x) - torch.log(mx)) / float(temperature)), torch.zeros_like(x))
    w = torch.nan_to_num(w, nan=0.0)
    keep = torch.ones(R, V, dtype=torch.bool)
    k = int(topK)
    if 1 <= k < V:
        kth = torch.topk(x, k, dim=1).values[:, -1:]
        keep &= x >= kth
    margin = torch.full((R,), float("inf"), dtype=torch.float64)
    if float(topP) < 1.0:
        for r in range(R):
            xs, order = torch.sort(torch.where(keep[r], x[r], torch.full_like(x[r], -1.0)), descending=True)
            ws = torch.where(xs >= 0, w[r][order], torch.zeros_like(xs))
            c = torch.cumsum(ws, 0)
            target = float(topP) * float(c[-1])
            last = torch.ones(V, dtype=torch.bool)               # last position of each run of equal values
            last[:-1] = xs[:-1] != xs[1:]
            valid = last & (xs >= 0)
            masses = c[valid]
            j = int(torch.nonzero(masses >= target)[0]) if bool((masses >= target).any()) else masses.numel() - 1
            t = xs[valid][j]
            keep[r] &= x[r] >= t
            margin[r] = (masses - target).abs().min()
    return keep, w, margin


def beam_step_reference(p, score, finished, length, eosToken=-1, padToken=0):
    """fp64 oracle of one beam-search step. p [B*W, V], score [B, W], finished [B, W], length [B, W].
    -> (parent int32 [B, W] as global rows, token int64 [B, W], score fp64 [B, W], finished uint8 [B, W],
    length int32 [B, W]), best first under (score descending, flat index w*V + v ascending)."""
    import numpy as np
    B, W = score.shape
    V = p.shape[1]
    x = torch.nan_to_num(p.detach().cpu().to(torch.float64), nan=0.0).clamp_min(0.0).reshape(B, W, V).numpy()
    sc = score.detach().cpu().to(torch.float64).numpy()
    fin = finished.detach().cpu().numpy().astype(bool)
    ln = length.detach().cpu().numpy()
    eos = -1 if eosToken is None else int(eosToken)
    out = [np.zeros((B, W), dt) for dt in (np.int32, np.int64, np.float64, np.uint8, np.int32)]
    for b in range(B):
        cs, ci = [], []
        for w in range(W):
            if fin[b, w]:
                cs.append(np.array([sc[b, w]]))
                ci.append(np.array([w * V + min(max(int(padToken), 0), V - 1)]))
            else:
                with np.errstate(divide="ignore"):
                    cs.append(sc[b, w] + np.log(x[b, w]))
                ci.append(w * V + np.arange(V))
        cs, ci = np.concatenate(cs), np.concatenate(ci)
        order = np.lexsort((ci, -cs))[:W]
        for j, o in enumerate(order):
            w, v = divmod(int(ci[o]), V)
            t = int(padToken) if fin[b, w] else v
            out[0][b, j] = b * W + w
            out[1][b, j] = t
            out[2][b, j] = cs[o]
            out[3][b, j] = 1 if (fin[b, w] or (eos >= 0 and t == eos)) else 0
            out[4][b, j] = ln[b, w] + (0 if fin[b, w] else 1)
    return tuple(torch.from_numpy(a) for a in out)


# ------------------------------------------------------------------------------------------------ torch paths
def _count(finished, count):
    if count is not None:
        count.copy_((finished == 0).sum().to(count.dtype).reshape(count.shape))


def sample_rows_torch(p, temperature=1.0, topK=0, topP=1.0, greedy=False, rng=None, finished=None, eosToken=-1,
                      padToken=0, count=None, advance=False):
    """Torch implementation of the row sampler (sums in fp64). Reads the counter of ``rng`` on the host."""
    R, V = p.shape
    x = torch.nan_to_num(p.float(), nan=0.0).clamp_min(0.0)
    rows = torch.arange(R, device=p.device)
    if greedy:
        tok = torch.argmax(x, dim=1)
        u = torch.zeros(R, dtype=torch.float32, device=p.device)
    else:
        mx = x.max(dim=1, keepdim=True).values
        w = torch.where(x > 0, torch.exp2((torch.log2(x) - torch.log2(mx)) / float(temperature)), torch.zeros_like(x))
        w = torch.nan_to_num(w, nan=0.0).double()
        keep = torch.ones_like(x, dtype=torch.bool)
        k = int(topK)
        if 1 <= k < V:
            keep &= x >= torch.topk(x, k, dim=1).values[:, -1:]
        if float(topP) < 1.0:
            xs, order = torch.sort(torch.where(keep, x, torch.full_like(x, -1.0)), dim=1, descending=True, stable=True)
            c = torch.cumsum(torch.where(xs >= 0, torch.gather(w, 1, order), torch.zeros_like(w)), 1)
            hit = (c >= float(topP) * c[:, -1:]) & (xs >= 0)
            j = torch.where(hit.any(1), hit.int().argmax(1), (xs >= 0).sum(1) - 1)
            keep &= x >= torch.gather(xs, 1, j.reshape(R, 1))
        wk = torch.where(keep, w, torch.zeros_like(w))
        cdf = torch.cumsum(wk, 1)
        u = sample_uniform(rng.seed, int(rng.offset.item()), R).to(p.device)
        target = u.double().reshape(R, 1) * cdf[:, -1:]
        pos = wk > 0
        hit = (cdf > target) & pos
        lastpos = (V - 1) - pos.flip(1).int().argmax(1)
        tok = torch.where(hit.any(1), hit.int().argmax(1), lastpos)
        dead = ~pos.any(1)                                       # an all-zero row: its argmax (index 0)
        tok = torch.where(dead, torch.zeros_like(tok), tok)
        u = torch.where(dead, torch.zeros_like(u), u)
        if advance:
            rng.advance()
    logp = torch.log(x[rows, tok])
    if finished is not None:
        done = finished != 0
        tok = torch.where(done, torch.full_like(tok, int(padToken)), tok)
        logp = torch.where(done, torch.zeros_like(logp), logp)
        u = torch.where(done, torch.zeros_like(u), u)
        if eosToken is not None and int(eosToken) >= 0:
            finished |= (tok == int(eosToken)).to(finished.dtype) & (~done).to(finished.dtype)
        _count(finished, count)
    return tok.to(torch.int64), logp.float(), u


def beam_step_torch(p, score, finished, length, eosToken=-1, padToken=0, count=None):
    """Torch implementation of the beam step; updates score / finished / length in place like the kernel.
    -> (parent int32 [B, W], token int64 [B, W])."""
    B, W = score.shape
    V = p.shape[1]
    x = torch.nan_to_num(p.float(), nan=0.0).clamp_min(0.0).reshape(B, W, V)
    fin = (finished != 0).reshape(B, W, 1)
    pad = min(max(int(padToken), 0), V - 1)
    cols = torch.arange(V, device=p.device).reshape(1, 1, V)
    cand = torch.where(fin, score.reshape(B, W, 1).expand(B, W, V), score.reshape(B, W, 1) + torch.log(x))
    valid = (~fin) | (cols == pad)
    cand = torch.where(valid, cand, torch.full_like(cand, _NEG_INF)).reshape(B, W * V)
    s1, o1 = torch.sort(cand, dim=1, descending=True, stable=True)
    v1 = torch.gather(valid.reshape(B, W * V), 1, o1)
    _, o2 = torch.sort((~v1).to(torch.int8), dim=1, stable=True)          # real candidates first, order kept
    top = o2[:, :W]
    idx = torch.gather(o1, 1, top)
    news = torch.gather(s1, 1, top)
    w = idx // V
    v = idx - w * V
    pf = torch.gather(finished.reshape(B, W) != 0, 1, w)
    tok = torch.where(pf, torch.full_like(v, int(padToken)), v)
    newf = pf | ((tok == int(eosToken)) if eosToken is not None and int(eosToken) >= 0 else torch.zeros_like(pf))
    newl = torch.gather(length.reshape(B, W), 1, w) + (~pf).to(length.dtype)
    parent = (torch.arange(B, device=p.device).reshape(B, 1) * W + w).to(torch.int32)
    score.copy_(news)
    finished.copy_(newf.to(finished.dtype))
    length.copy_(newl)
    _count(finished, count)
    return parent, tok.to(torch.int64)


def cache_gather_torch(src, dst, parent, L):
    """dst[i, :L] = src[parent[i], :L] by index_select."""
    dst[:, :L] = src.index_select(0, parent.to(torch.int64))[:, :L]
    return dst


# ------------------------------------------------------------------------------------------------ kernels
def sample_rows_native(p, temperature=1.0, topK=0, topP=1.0, greedy=False, rng=None, finished=None, eosToken=-1,
                       padToken=0, count=None, want_u=False, out=None, advance=False):
    """Row sampler on csrc/generation.hip; None when the kernel refuses. ``out``: optional (tok, logp) to write."""
    R, V = p.shape
    if out is None:
        tok = torch.empty(R, dtype=torch.int64, device=p.device)
        logp = torch.empty(R, dtype=torch.float32, device=p.device)
    else:
        tok, logp = out
    u = torch.empty(R, dtype=torch.float32, device=p.device) if want_u else None
    rc = native.load().dl4j_gen_sample_dt(
        _DT[p.dtype], _ptr(p), R, V, float(temperature), int(topK), float(topP), int(bool(greedy)),
        0 if rng is None else rng.seed, None if rng is None else _ptr(rng.offset), int(bool(advance)), _ptr(tok),
        _ptr(logp), _ptr(u),
        _ptr(finished), -1 if eosToken is None else int(eosToken), int(padToken), _ptr(count), _stream())
    if rc == -1:
        return None
    _check(rc, "gen_sample")
    return tok, logp, u


def beam_step_native(p, score, finished, length, eosToken=-1, padToken=0, count=None, out=None):
    """Beam step on csrc/generation.hip; None when the kernel refuses. ``out``: optional (parent, token)."""
    B, W = score.shape
    if out is None:
        parent = torch.empty(B, W, dtype=torch.int32, device=p.device)
        token = torch.empty(B, W, dtype=torch.int64, device=p.device)
    else:
        parent, token = out
    rc = native.load().dl4j_gen_beam_step_dt(
        _DT[p.dtype], _ptr(p), B, W, p.shape[1], _ptr(score), _ptr(finished), _ptr(length), _ptr(parent), _ptr(token),
        -1 if eosToken is None else int(eosToken), int(padToken), _ptr(count), _stream())
    if rc == -1:
        return None
    _check(rc, "gen_beam_step")
    return parent, token


def cache_gather_native(src, dst, parent, L):
    """dst[i, :L] = src[parent[i], :L] on csrc/generation.hip (src [mbS, TcapS, C], dst [mbD, TcapD, C], parent int32
    [mbD] on the device). -> dst, or None (nothing written) when the kernel refuses: not contiguous, not 16-byte
    aligned, a row that is no multiple of 16 bytes, src and dst the same buffer."""
    if not (src.is_cuda and dst.is_cuda and parent.is_cuda and src.dim() == 3 and dst.dim() == 3 and
            src.dtype == dst.dtype and src.is_contiguous() and dst.is_contiguous() and
            parent.dtype == torch.int32 and parent.is_contiguous() and parent.numel() == dst.shape[0] and
            src.shape[2] == dst.shape[2] and src.element_size() in (1, 2, 4)):
        return None
    rc = native.load().dl4j_gen_cache_gather(_ptr(src), _ptr(dst), _ptr(parent), src.shape[0], dst.shape[0],
                                             src.shape[1], dst.shape[1], int(L), src.shape[2], src.element_size(),
                                             _stream())
    if rc == -1:
        return None
    _check(rc, "gen_cache_gather")
    return dst


# ------------------------------------------------------------------------------------------------ dispatch
def sample_rows(p, temperature=1.0, topK=0, topP=1.0, greedy=False, rng=None, finished=None, eosToken=-1,
                padToken=0, count=None, out=None, advance=False):
    """One token per row of the probabilities p [R, V] -> (tok int64 [R], logp fp32 [R]). ``finished`` (uint8 [R]) is
    updated in place and ``count`` (int32 [1]) receives the number of unfinished rows; ``advance`` bumps the counter
    of ``rng`` after the draw (on the device)."""
    if _kernel_ok(p):
        r = sample_rows_native(p, temperature, topK, topP, greedy, rng, finished, eosToken, padToken, count, out=out,
                               advance=advance)
        if r is not None:
            return r[0], r[1]
    fallback.note(p, "generation", f"sampler on {p.dtype}: torch path")
    tok, logp, _ = sample_rows_torch(p, temperature, topK, topP, greedy, rng, finished, eosToken, padToken, count,
                                     advance)
    if out is not None:
        out[0].copy_(tok)
        out[1].copy_(logp)
        return out
    return tok, logp


def beam_step(p, score, finished, length, eosToken=-1, padToken=0, count=None, out=None):
    """One beam-search step -> (parent int32 [B, W], token int64 [B, W]); score / finished / length in place."""
    if _kernel_ok(p) and 1 <= score.shape[1] <= 16:
        r = beam_step_native(p, score, finished, length, eosToken, padToken, count, out=out)
        if r is not None:
            return r
    fallback.note(p, "generation", f"beam step on {p.dtype}: torch path")
    return beam_step_torch(p, score, finished, length, eosToken, padToken, count)


def cache_gather(src, dst, parent, L):
    """dst[i, :L] = src[parent[i], :L]; the kernel where it takes the operands, else index_select."""
    if use_native(src, "generation") and cache_gather_native(src, dst, parent, L) is not None:
        return dst
    fallback.note(src, "generation", f"cache gather on {src.dtype} {tuple(src.shape)}: index_select")
    return cache_gather_torch(src, dst, parent, L)


def step_commit_torch(short=None, record=None):
    """Torch implementation of the step commit (reads the step counter on the host)."""
    if short is not None:
        short.copy_((short - 1).clamp_(min=0))
    if record is not None:
        step, stok, slogp, tokens, logps = record
        t = int(step.item())
        if 0 <= t < tokens.shape[0]:
            tokens[t].copy_(stok)
            logps[t].copy_(slogp)
            step.add_(1)


def step_commit(short=None, record=None):
    """The bookkeeping of one pinned generation step in one call with constant arguments (csrc/generation.hip):
    ``short`` (int32 [mb] on the device, or None) drops by one per row, not below 0; ``record`` = (step int32 [1],
    stok int64 [rows], slogp fp32 [rows], tokens int64 [N, rows], logps fp32 [N, rows]) or None files the staged
    token / log-probability as row ``step`` of the result buffers and bumps ``step`` (nothing once step >= N)."""
    if short is None and record is None:
        return
    ref = short if short is not None else record[0]
    ok = use_native(ref, "generation")
    if ok and short is not None:
        ok = short.dtype == torch.int32 and short.dim() == 1 and short.is_contiguous() and short.numel() >= 1
    if ok and record is not None:
        step, stok, slogp, tokens, logps = record
        N, rows = tokens.shape
        ok = (step.dtype == torch.int32 and step.numel() == 1 and stok.dtype == tokens.dtype == torch.int64 and
              slogp.dtype == logps.dtype == torch.float32 and stok.shape == slogp.shape == (rows,) and
              logps.shape == tokens.shape and N >= 1 and rows >= 1 and
              all(t.is_contiguous() and t.device == ref.device for t in record))
    if ok:
        step, stok, slogp, tokens, logps = record if record is not None else (None,) * 5
        rc = native.load().dl4j_gen_step_commit(
            _ptr(short), 0 if short is None else short.numel(), _ptr(step), _ptr(stok), _ptr(slogp), _ptr(tokens),
            _ptr(logps), 0 if record is None else tokens.shape[1], 0 if record is None else tokens.shape[0],
            _stream())
        if rc != -1:
            _check(rc, "gen_step_commit")
            return
    fallback.note(ref, "generation", "step commit: torch path")
    step_commit_torch(short, record)


def beam_backtrack(toks, parents, best, W):
    """The token sequence of each example's chosen beam: toks [N, mb*W] int64 and parents [N, mb*W] int32 as the beam
    steps wrote them, best [mb] (the final beam per example) -> [mb, N] int64. One kernel launch on the GPU."""
    N, rows = toks.shape
    mb = rows // W
    best = best.to(torch.int64).contiguous()
    out = torch.empty(mb, N, dtype=torch.int64, device=toks.device)
    if use_native(toks, "generation") and toks.is_contiguous() and parents.is_contiguous() and \
            parents.dtype == torch.int32:
        rc = native.load().dl4j_gen_beam_backtrack(_ptr(toks), _ptr(parents), _ptr(best), _ptr(out), mb, W, N,
                                                   _stream())
        if rc != -1:
            _check(rc, "gen_beam_backtrack")
            return out
    fallback.note(toks, "generation", "beam backtrack: torch path")
    r = torch.arange(mb, device=toks.device) * W + best
    for t in range(N - 1, -1, -1):
        out[:, t] = toks[t][r]
        r = parents[t][r].to(torch.int64)
    return out


# ------------------------------------------------------------------------------------------------ speculative decoding
# csrc/speculative.hip: the semantics are written out at the top of that file. The operands of the three ops are
# updated in place, by the kernels and by their torch twins alike.
SPEC_PHILOX_TAG = 0x53504543


def spec_uniform(seed, offset, rows, K):
    """The verify step's uniforms at counter value ``offset``: fp32 [rows, 2K+2] in [0, 1), slot s of row r from 24
    bits of word 0 of philox4x32_10({r, s, SPEC_PHILOX_TAG, offset mod 2^32}, {seed low, seed high}); slot 2i decides
    draft i, slot 2i+1 draws the token that replaces it (2K+1: the token after K accepted drafts)."""
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    off = int(offset) & 0xFFFFFFFF
    return torch.tensor([[(philox4x32_10((r, s, SPEC_PHILOX_TAG, off), key)[0] >> 8) / 16777216.0
                          for s in range(2 * int(K) + 2)] for r in range(int(rows))], dtype=torch.float32)


def _tempered(x, invT):
    """fp64 weights (x / max)^(1/T) of the rows of x [R, V] (cleaned probabilities) -> (w, row sums)."""
    mx = x.max(dim=1, keepdim=True).values
    lm = torch.where(mx > 0, torch.log2(mx), torch.zeros_like(mx))
    w = torch.where(x > 0, torch.exp2((torch.log2(x) - lm) * invT), torch.zeros_like(x))
    w = torch.nan_to_num(w, nan=0.0)
    return w, w.sum(1)


def spec_verify_torch(p, q, d, u, temperature, greedy, length, cursor, finished, eosToken, padToken, tokens, logps,
                      nxt, next2=None, hist=None, counters=None, diag=None):
    """Torch implementation of the verify step (sums in fp64, vectorised over the rows). p [mb, K+1, V] and q
    [mb, K, V] (or None) probabilities, d int64 [mb, K], u [mb, 2K+2] the uniforms (``spec_uniform``); length /
    cursor int32 [mb], finished uint8 [mb], tokens int64 [mb, N], logps fp32 [mb, N], nxt int64 [mb], next2 (a [mb]
    view), hist int64 [mb, Hcap] and counters int32 [2] are updated in place. ``diag``: a dict that receives
    ``"risky"`` bool [mb]: rows with an accept decision closer than 1e-5 * p~(d), or a draw within 1e-5 of the mass
    from a boundary of its token's range — decisions that fp32 sums may resolve either way."""
    mb, K1, V = p.shape
    K, N, dev = K1 - 1, tokens.shape[1], p.device
    eos = -1 if eosToken is None else int(eosToken)
    invT = 1.0 if greedy else 1.0 / float(temperature)
    x32 = torch.nan_to_num(p.float(), nan=0.0).clamp_min(0.0)
    xq32 = None if q is None else torch.nan_to_num(q.float(), nan=0.0).clamp_min(0.0)
    ud = u.to(device=dev, dtype=torch.float64)
    rows = torch.arange(mb, device=dev)
    cur0 = cursor.to(torch.int64)
    active = (finished == 0) & (cur0 < N) & (cur0 >= 0)
    cur, L = cur0.clone(), length.to(torch.int64)
    emitted = torch.zeros(mb, dtype=torch.int64, device=dev)
    nacc = torch.zeros_like(emitted)
    last = torch.full_like(emitted, int(padToken))
    fin_new = torch.zeros(mb, dtype=torch.bool, device=dev)
    risky = torch.zeros(mb, dtype=torch.bool, device=dev)
    run = active.clone()
    for i in range(K + 1):
        if not bool(run.any()):
            break
        bonus = i == K
        xp = x32[:, i].double()
        pmax, amax = xp.max(1).values, torch.argmax(xp, dim=1)
        di = torch.full_like(cur, -1) if bonus else d[:, i].to(torch.int64)
        valid = (di >= 0) & (di < V)
        dd = torch.where(valid, di, torch.full_like(di, -1))
        dc = dd.clamp(min=0).reshape(mb, 1)
        if greedy:
            accepted = (dd == amax) & (not bonus)
            tok = amax
        else:
            wp, Sp = _tempered(xp, invT)
            if bonus:
                accepted = torch.zeros(mb, dtype=torch.bool, device=dev)
                mass = wp
            else:
                if xq32 is None:
                    xq = torch.zeros_like(xp).scatter_(1, dc, valid.double().reshape(mb, 1))
                else:
                    xq = xq32[:, i].double()
                wq, Sq = _tempered(xq, invT)
                wpd = wp.gather(1, dc)[:, 0] * valid
                wqd = wq.gather(1, dc)[:, 0] if xq32 is not None else torch.ones_like(wpd)
                lhs, rhs = ud[:, 2 * i] * wqd * Sp, wpd * Sq
                accepted = (lhs < rhs) & valid
                risky |= run & valid & ((lhs - rhs).abs() < 1e-5 * rhs)
                res = (wp * Sq.reshape(mb, 1) - wq * Sp.reshape(mb, 1)).clamp_min(0.0)
                mass = torch.where((res.sum(1) > 0).reshape(mb, 1), res, wp)
            cdf = torch.cumsum(mass, 1)
            total = cdf[:, -1]
            target = ud[:, 2 * i + 1] * total
            pos = mass > 0
            hit = (cdf > target.reshape(mb, 1)) & pos
            lastpos = (V - 1) - pos.flip(1).int().argmax(1)
            draw = torch.where(hit.any(1), hit.int().argmax(1), lastpos)
            draw = torch.where(pos.any(1), draw, amax)
            lo = torch.where(draw > 0, cdf.gather(1, (draw - 1).clamp(min=0).reshape(mb, 1))[:, 0],
                             torch.zeros_like(total))
            hi = cdf.gather(1, draw.reshape(mb, 1))[:, 0]
            near = ((target - lo).abs() < 1e-5 * total) & (draw > 0) | ((target - hi).abs() < 1e-5 * total)
            risky |= run & ~accepted & near & (pmax > 0)
            tok = torch.where(accepted, dd, draw)
            zero = ~(pmax > 0)                                   # nothing to draw from: the argmax (index 0)
            accepted = accepted & ~zero
            tok = torch.where(zero, amax, tok)
        r = rows[run]
        t = tok[run]
        tokens[r, cur[run]] = t
        logps[r, cur[run]] = torch.log(x32[r, i, t])
        if hist is not None:
            at = L[run] + 1 + emitted[run]
            ok = at < hist.shape[1]
            hist[r[ok], at[ok]] = t[ok]
        cur = cur + run
        emitted = emitted + run
        last = torch.where(run, tok, last)
        nacc = nacc + (run & accepted)
        done = (tok == eos) | (cur >= N)
        fin_new |= run & done
        run = run & accepted & ~done
    if counters is not None:
        drafted = torch.minimum(torch.full_like(cur0, K), N - cur0)
        counters[0] += int(drafted[active].sum())
        counters[1] += int(nacc[active].sum())
    cursor.copy_(torch.where(active, cur, cur0).to(cursor.dtype))
    length.copy_((L + emitted).to(length.dtype))
    finished.copy_(torch.where(active, fin_new, torch.ones_like(fin_new)).to(finished.dtype))
    nxt.copy_(last)
    if next2 is not None:
        next2.copy_(last)
    if diag is not None:
        diag["risky"] = risky


def spec_commit_torch(length, finished, short, slot):
    """Torch implementation of the commit: short = max(length) - length, slot = (rows not finished, max(length))."""
    m = length.max()
    short.copy_(m - length)
    slot[0] = (finished == 0).sum()
    slot[1] = m


def ngram_draft_torch(hist, length, ngram, K, d):
    """Torch implementation of the prompt-lookup draft (host loops): d [mb, K] int64 (any strides) in place."""
    H = hist.cpu()
    for b, L in enumerate(length.tolist()):
        h = H[b].tolist()
        L = min(max(int(L), 0), len(h) - 1)
        j = -1
        for n in range(int(ngram), 0, -1):
            if L - n + 1 < 0:
                continue
            tail = h[L - n + 1:L + 1]
            j = max((e for e in range(n - 1, L) if h[e - n + 1:e + 1] == tail), default=-1)
            if j >= 0:
                break
        d[b] = torch.tensor([h[j + 1 + (i % (L - j))] if j >= 0 else h[L] for i in range(int(K))], dtype=torch.int64)
    return d


def _rows3(t):
    """t [mb, R, V] (any row strides, unit stride in V) -> (time stride, batch stride) in elements, or None."""
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1) or t.stride(0) < 0 or t.stride(1) < 0:
        return None
    return t.stride(1), t.stride(0)


def spec_verify_native(p, q, d, temperature, greedy, rng, length, cursor, finished, eosToken, padToken, tokens, logps,
                       nxt, next2=None, hist=None, counters=None, want_u=False, advance=False):
    """The verify step on csrc/speculative.hip, operands as ``spec_verify_torch`` (p / q are read where they lie, by
    their strides; rng: the PhiloxStream whose counter the draws use). -> the uniforms [mb, 2K+2] with ``want_u``, else
    True; None when the kernel refuses."""
    mb, K1, V = p.shape
    K = K1 - 1
    ps, qs = _rows3(p), (0, 0) if q is None else _rows3(q)
    ints = (length, cursor)
    if ps is None or qs is None or p.dtype not in _DT or (q is not None and (q.dtype != p.dtype or
                                                                               tuple(q.shape) != (mb, K, V))):
        return None
    if not (d.dtype == torch.int64 and tuple(d.shape) == (mb, K) and tokens.dtype == torch.int64 and
            logps.dtype == torch.float32 and tokens.shape == logps.shape and tokens.shape[0] == mb and
            tokens.is_contiguous() and logps.is_contiguous() and nxt.dtype == torch.int64 and nxt.is_contiguous() and
            nxt.numel() == mb and finished.dtype == torch.uint8 and finished.is_contiguous() and
            all(t.dtype == torch.int32 and t.is_contiguous() and t.numel() == mb for t in ints)):
        return None
    if next2 is not None and not (next2.dtype == torch.int64 and tuple(next2.shape) == (mb,)):
        return None
    if hist is not None and not (hist.dtype == torch.int64 and hist.dim() == 2 and hist.shape[0] == mb and
                                 hist.is_contiguous()):
        return None
    if counters is not None and not (counters.dtype == torch.int32 and counters.numel() == 2 and
                                     counters.is_contiguous()):
        return None
    u = torch.empty(mb, 2 * K + 2, dtype=torch.float32, device=p.device) if want_u else None
    rc = native.load().dl4j_spec_verify_dt(
        _DT[p.dtype], _ptr(p), ps[0], ps[1], _ptr(q), qs[0], qs[1], _ptr(d), d.stride(0), d.stride(1), mb, K, V,
        float(temperature), int(bool(greedy)), 0 if rng is None else rng.seed,
        None if rng is None else _ptr(rng.offset), int(bool(advance)), _ptr(length), _ptr(cursor), _ptr(finished),
        -1 if eosToken is None else int(eosToken), int(padToken), tokens.shape[1], _ptr(tokens), _ptr(logps),
        _ptr(nxt), _ptr(next2), 0 if next2 is None else next2.stride(0), _ptr(hist),
        0 if hist is None else hist.shape[1], _ptr(counters), _ptr(u), _stream())
    if rc == -1:
        return None
    _check(rc, "spec_verify")
    return u if want_u else True


def spec_verify(p, q, d, temperature, greedy, rng, length, cursor, finished, eosToken, padToken, tokens, logps, nxt,
                next2=None, hist=None, counters=None):
    """Check the K drafted tokens d [mb, K] against the target's distributions p [mb, K+1, V] (q [mb, K, V]: the
    distributions they were drawn from, None for deterministic drafts): every row emits its accepted drafts and one
    more token into tokens / logps at its cursor; length, cursor, finished, nxt (and next2, hist, counters) are
    updated in place and the counter of ``rng`` advances after the draws."""
    if use_native(p, "generation") and p.numel() < 2 ** 31 and \
            spec_verify_native(p, q, d, temperature, greedy, rng, length, cursor, finished, eosToken, padToken,
                               tokens, logps, nxt, next2, hist, counters, advance=True) is not None:
        return
    fallback.note(p, "generation", f"speculative verify on {p.dtype}: torch path")
    K = p.shape[1] - 1
    if greedy:
        u = torch.zeros(p.shape[0], 2 * K + 2)
    else:
        u = spec_uniform(rng.seed, int(rng.offset.item()), p.shape[0], K)
        rng.advance()
    spec_verify_torch(p, q, d, u, temperature, greedy, length, cursor, finished, eosToken, padToken, tokens, logps,
                      nxt, next2, hist, counters)


def spec_commit(length, finished, short, slot):
    """After a verify step: short int32 [mb] = max(length) - length (the shortfall array the cached layers share) and
    slot int32 [2] = (rows not finished, max(length)), what the host reads once per round."""
    if use_native(length, "generation") and all(t.is_contiguous() for t in (length, finished, short, slot)) and \
            length.dtype == short.dtype == slot.dtype == torch.int32 and finished.dtype == torch.uint8 and \
            length.numel() == finished.numel() == short.numel() and slot.numel() == 2:
        rc = native.load().dl4j_spec_commit(_ptr(length), _ptr(finished), length.numel(), _ptr(short), _ptr(slot),
                                            _stream())
        if rc != -1:
            _check(rc, "spec_commit")
            return
    fallback.note(length, "generation", "speculative commit: torch path")
    spec_commit_torch(length, finished, short, slot)


def ngram_draft_native(hist, length, ngram, K, d):
    """The prompt-lookup draft on csrc/speculative.hip; None when the kernel refuses."""
    mb = hist.shape[0]
    if not (hist.dim() == 2 and hist.dtype == torch.int64 and hist.is_contiguous() and length.dtype == torch.int32 and
            length.is_contiguous() and length.numel() == mb and d.dtype == torch.int64 and
            tuple(d.shape) == (mb, int(K)) and d.stride(0) >= 0 and d.stride(1) >= 0):
        return None
    rc = native.load().dl4j_spec_ngram_draft(_ptr(hist), hist.shape[1], _ptr(length), mb, int(ngram), int(K), _ptr(d),
                                             d.stride(0), d.stride(1), _stream())
    if rc == -1:
        return None
    _check(rc, "spec_ngram_draft")
    return d


def ngram_draft(hist, length, ngram, K, d):
    """Prompt lookup: row b's history is hist[b, 0 .. length[b]] (the last entry: the token not yet fed); d [mb, K]
    receives the continuation of the latest earlier occurrence of its last ``ngram`` (down to 1) tokens, extended
    periodically, or K copies of the last token without one."""
    if use_native(hist, "generation") and ngram_draft_native(hist, length, ngram, K, d) is not None:
        return d
    fallback.note(hist, "generation", "n-gram draft: torch path")
    return ngram_draft_torch(hist, length, ngram, K, d)


def spec_keep(src, dst, tok=None, tokDst=None):
    """dst[b] = src[b] for the rows of an assistant's distribution src [mb, V] (dst: a [mb, V] view with unit stride
    in V) and tokDst[b] = tok[b] (int64; tokDst any [mb] view): one launch of csrc/speculative.hip, else copy_."""
    if use_native(src, "generation") and src.dtype in _DT and src.dtype == dst.dtype and src.is_contiguous() and \
            src.dim() == 2 and dst.shape == src.shape and (src.shape[1] == 1 or dst.stride(1) == 1) and \
            (tok is None or (tok.dtype == tokDst.dtype == torch.int64 and tok.is_contiguous() and
                             tok.numel() == tokDst.numel() == src.shape[0] and tokDst.dim() == 1)):
        rc = native.load().dl4j_spec_keep_dt(_DT[src.dtype], _ptr(src), _ptr(dst), dst.stride(0), src.shape[0],
                                             src.shape[1], _ptr(tok), _ptr(tokDst),
                                             0 if tok is None else tokDst.stride(0), _stream())
        if rc != -1:
            _check(rc, "spec_keep")
            return
    fallback.note(src, "generation", "speculative keep: torch path")
    dst.copy_(src)
    if tok is not None:
        tokDst.copy_(tok)
