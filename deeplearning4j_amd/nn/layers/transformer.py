"""Transformer runtime layers: BERT embeddings, post-LN encoder block, [CLS] pooler.

Not in the reference snapshot (no attention or LayerNorm there); they implement the BERT-base
config of BASELINE.json on the same layer SPI (activate / backpropGradient writing into flat gradient views).

MI355X structure of one encoder block (token-major [B*T, E] activations, bf16 compute, fp32 master weights):
  qkv = x·Wqkv + b          one fused projection GEMM (in-tree MFMA GEMM, bias in the epilogue)
  ctx = attention(qkv)      flash-style HIP kernel reading Q/K/V in place (csrc/attention.hip)
  h1  = LN(ctx·Wo + bo + x) output GEMM + LayerNorm-with-residual HIP kernel (csrc/layernorm.hip)
  h2  = LN(gelu(h1·W1 + b1)·W2 + b2 + h1)
The backward is written out by hand (no autograd): GEMMs produce fp32 weight gradients straight into the flat
gradient views, attention/LN backward are the matching HIP kernels, and the residual gradients are summed in
place. Activations cross layer boundaries as [mb, E, T] *views* of token-major memory, so stacking blocks costs
no transposes. On CPU (and fp64 gradient checks) the same math runs on plain torch ops.

Dropout (training only; ``hiddenDropout`` / ``attentionDropout`` are DROP probabilities, 0 = off = the path above):
  ctx = attention(qkv) with the keep mask generated inside the flash kernels (csrc/attention.hip, DROP instances)
  h1  = LN(drop(ctx·Wo + bo) + x),  h2 = LN(drop(ffn) + h1): the mask is applied by the LayerNorm forward kernel as
        it loads its input (which it overwrites with the dropped values, the x of the unchanged LayerNorm backward)
Backward of a hidden site: ds from the LayerNorm backward is the residual's gradient; the producer's is ds∘D, one
launch of the Philox dropout kernel in backward mode (it regenerates the mask), and the producer's bias gradient is
the column sum of ds∘D by the column-sum kernel — the dropout is NOT fused into the LayerNorm backward kernels.
Each layer owns one PhiloxStream advanced once per training forward; its sites use keys derived from the layer's
seed. Off the kernels (CPU, fp32 / fp64, other head sizes) the masks come from ``dropoutKeep``.

Generation (``rnnTimeStep``): a causal block keeps a key/value cache (``KVCacheState``): the new chunk is projected,
its K / V appended, its queries attend over the cache (csrc/attention_decode.hip, or the torch reference off the
kernels) and the rest of the block runs as in the inference forward; the embedding layer continues its positions.
A bidirectional block cannot stream and runs ``activate`` on the chunk.

Grouped-query attention (``nKVHeads`` on the encoder block): Wqkv projects to [B*T, E + 2*Ekv] (Q | K | V with the
nKVHeads key/value heads only), the flash kernels share each of them between the query heads of its group, the
backward returns dK / dV summed over the group, and the cache holds 2*Ekv columns (or the fp8 rows of nKVHeads heads).

Rotary position embeddings (``positionEncoding="rotary"`` on the encoder block): the Q and K columns of qkv are
rotated by their positions right after the projection (csrc/attention_rope.hip, in place), the rotated qkv is what the
attention reads and the backward keeps, and the transposed rotation runs on dQ | dK before the weight, bias and input
gradients. In ``rnnTimeStep`` a token's position is the index of its cache row and the append launch rotates as it
stores, so the cache holds rotated keys and a step gains no launch. ``BertEmbeddingLayer.positionEmbeddings(False)``
drops the learned position table (and with it the limit on a generated sequence's length).

Llama-style block (``normalization="rms"``, ``normPlacement="pre"`` on the encoder block; ``ffnActivation="swiglu"`` in
either block): n1 = rms(x), a = Attn(n1)·Wo + bo, (h, n2) = rms(a, r = x) in ONE launch that overwrites a with
h = x + a (csrc/rmsnorm.hip), f = swiglu(n2·W1 + b1) (csrc/swiglu.hip; or the GELU epilogue), y = h + f·W2 + b2 (the
add rides on the GEMM in ``rnnTimeStep`` and is one pairwise launch in ``activate``). Backward mirrors it: the norm's
backward kernel takes the gradient arriving over the residual path as ``dres`` and adds it before the one rounding.
Hidden dropout uses the stand-alone Philox launches on the two branch outputs.

Mixture-of-experts feed-forward (``nExperts`` on the encoder block): logits = n·Wr in fp32 (n: the feed-forward's input),
the router picks k experts per token and sorts the (token, choice) assignments by expert on the device (csrc/moe.hip),
Xp = gather(n), Z1p = Xp·W1[e] + b1[e] and Yp = act(Z1p)·W2[e] + b2[e] on the grouped mode of the GEMM (every 128-row
tile reads its own expert's matrix), f2[n] = sum_j g_j·Yp[row(n, j)] in fp32 (the last add of a pre-norm ``rnnTimeStep``
rides on this launch). Backward: the gate gradients by wave dot products, dYp = g·df2 gathered, the per-expert weight
gradients over the segments' live rows straight into the gradient views, and the router's gradient through the plain
GEMMs. Every launch is sized by shapes alone and nothing is read back, so a step captures into a graph as it is.

Decoder block (``TransformerDecoderLayerImpl``, a two-input graph layer: decoder stream + encoder memory): causal
self-attention as above, then cross-attention of q2 = h1·Wq2 over kv2 = memory·Wkv2 (one GEMM straight into the
kv [mb, Tk, 2E] layout of csrc/attention_cross.hip), then the FFN, each followed by LayerNorm(+residual). Its
``rnnTimeStep`` keeps kv2 and the memory's mask (``MemoryKVState``) next to the self-attention cache.
"""
import math

import torch
import torch.nn.functional as F

from ... import ops
from .base import LayerImpl, copy_grad_, matmul, weight_grad_
from ...ops.gemm import bias_vec, mmul


def _native(x, op):
    return x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and ops.use_native(x, op)


def _wgrad(view, a, b):
    """view <- aᵀ·b on the in-tree GEMM: fp32 accumulation written straight into the fp32 gradient view."""
    weight_grad_(view, a.t(), b)


def _bsum(view, d):
    """view <- column sums of d, accumulated in the view's precision without a converted copy of d."""
    if d.is_cuda and view.is_contiguous() and view.dtype == torch.float32 and ops.use_native(d, "bias_grad"):
        from ...ops import native
        if native.channel_sum(d.contiguous(), out=view.view(-1)) is not None:
            return
    if view.is_contiguous():
        torch.sum(d, 0, dtype=view.dtype, out=view.view(-1))
    else:
        copy_grad_(view, d.sum(0, dtype=view.dtype))


def _gelu_fwd(z):
    if _native(z, "gelu"):
        from ...ops import transformer_native as TN
        r = TN.gelu(z)
        if r is not None:
            return r
    return F.gelu(z)


def _gelu_bwd(z, dy):
    if _native(z, "gelu"):
        from ...ops import transformer_native as TN
        r = TN.gelu(z, dy.to(z.dtype).contiguous())
        if r is not None:
            return r
    zf = z.float() if z.dtype != torch.float64 else z
    cdf = 0.5 * (1.0 + torch.erf(zf * (1.0 / math.sqrt(2.0))))
    pdf = torch.exp(-0.5 * zf * zf) * (1.0 / math.sqrt(2.0 * math.pi))
    return (dy.to(zf.dtype) * (cdf + zf * pdf)).to(z.dtype)


# ------------------------------------------------------------------------------------------------ LN helpers
def _ln_fwd(x, res, g, b, eps):
    if _native(x, "layernorm"):
        from ...ops import transformer_native as TN
        r = TN.ln_fwd(x, g, b, eps, res)
        if r is not None:
            y, mean, rstd = r
            return y, ("native", mean, rstd)
    s = x if res is None else x + res
    sf = s.float() if s.dtype != torch.float64 else s
    mean = sf.mean(-1, keepdim=True)
    rstd = torch.rsqrt(sf.var(-1, unbiased=False, keepdim=True) + eps)
    xhat = (sf - mean) * rstd
    y = xhat * g.reshape(-1).to(sf.dtype) + b.reshape(-1).to(sf.dtype)
    return y.to(x.dtype), ("torch", xhat, rstd)


def _ln_bwd(dy, x, res, g, ctx, gview=None, bview=None, dsum_view=None):
    """-> ds (gradient of x and of res); dgamma / dbeta land in the gradient views. ``dsum_view``: the producing dense
    layer's bias-gradient view, filled with the column sums of ds by the LayerNorm backward kernel itself when it
    can (returns with ``dsum_view`` handled), else by _bsum."""
    if ctx[0] == "native":
        from ...ops import transformer_native as TN
        dsv = dsum_view.view(-1) if dsum_view is not None and dsum_view.is_contiguous() and \
            dsum_view.dtype == torch.float32 else None
        ds, dg, db = TN.ln_bwd(dy, x, g, ctx[1], ctx[2], res, gview, bview, dsv)
        if dg.data_ptr() != gview.data_ptr():
            copy_grad_(gview, dg)
        if db.data_ptr() != bview.data_ptr():
            copy_grad_(bview, db)
        if dsum_view is not None and dsv is None:
            _bsum(dsum_view, ds)
        return ds
    _, xhat, rstd = ctx
    d = dy.to(xhat.dtype)
    dg = (d * xhat).sum(0)
    db = d.sum(0)
    dxh = d * g.reshape(-1).to(xhat.dtype)
    ds = rstd * (dxh - dxh.mean(-1, keepdim=True) - xhat * (dxh * xhat).mean(-1, keepdim=True))
    copy_grad_(gview, dg)
    copy_grad_(bview, db)
    ds = ds.to(x.dtype)
    if dsum_view is not None:
        _bsum(dsum_view, ds)
    return ds


# ------------------------------------------------------------------------------------------------ RMSNorm / SwiGLU
def _rms_fwd(x, res, g, eps, s_out=None):
    """RMSNorm of s = x (+ res) -> (y, s, rstd): csrc/rmsnorm.hip on a GPU in bf16 / fp16 (with ``res`` the add runs in
    the same launch and s is written to ``s_out``, which may be x itself), else ``rms_norm_reference``, counted as a
    fallback on a GPU."""
    from ...ops import transformer_native as TN
    if _native(x, "rmsnorm"):
        r = TN.rms_fwd(x, g, eps, res, s_out)
        if r is not None:
            return r
    if x.is_cuda:
        from ...ops import fallback
        fallback.record("rmsnorm", f"width {x.shape[-1]} / dtype {x.dtype}: torch reference path")
    return TN.rms_norm_reference(x, g, eps, res)


def _rms_bwd(dy, s, g, rstd, gview, dres=None, dsum_view=None, dx_out=None):
    """-> ds = the gradient of s (+ ``dres``, the gradient arriving over the residual path, added before the one
    rounding; ``dx_out`` may be ``dres``); dgamma lands in ``gview``. ``dsum_view``: the producing dense layer's
    bias-gradient view, filled with the column sums of ds by the backward kernel itself when it can, else by _bsum."""
    from ...ops import transformer_native as TN
    if _native(s, "rmsnorm") and rstd.dim() == 1:
        f32v = lambda v: v is not None and v.is_contiguous() and v.dtype == torch.float32  # noqa: E731
        dsv = dsum_view.view(-1) if f32v(dsum_view) else None
        r = TN.rms_bwd(dy.to(s.dtype).contiguous(), s, g, rstd, dres, gview.view(-1) if f32v(gview) else None, dsv,
                       dx_out)
        if r is not None:
            ds, dg = r
            if dg.data_ptr() != gview.data_ptr():
                copy_grad_(gview, dg)
            if dsum_view is not None and dsv is None:
                _bsum(dsum_view, ds)
            return ds
    ds, dg = TN.rms_norm_backward_reference(dy, s, g, rstd.reshape(-1, 1) if rstd.dim() == 1 else rstd, dres)
    copy_grad_(gview, dg)
    if dsum_view is not None:
        _bsum(dsum_view, ds)
    return ds


def _swiglu_fwd(z):
    """silu(gate) * up of the fused projection z [M, 2F] (csrc/swiglu.hip; ``swiglu_reference`` off the kernels,
    counted as a fallback on a GPU)."""
    from ...ops import transformer_native as TN
    if _native(z, "swiglu"):
        r = TN.swiglu(z)
        if r is not None:
            return r
    if z.is_cuda:
        from ...ops import fallback
        fallback.record("swiglu", f"width {z.shape[-1]} / dtype {z.dtype}: torch reference path")
    return TN.swiglu_reference(z)


def _swiglu_bwd(z, df):
    from ...ops import transformer_native as TN
    if _native(z, "swiglu"):
        r = TN.swiglu_bwd(z, df.to(z.dtype).contiguous())
        if r is not None:
            return r
    return TN.swiglu_backward_reference(z, df)


# ------------------------------------------------------------------------------------------------ mixture of experts
def _moe_op(name, like, *args, **kw):
    """``ops.transformer_native.<name>`` (csrc/moe.hip, the grouped GEMM) when ``like`` is on a GPU in bf16 / fp16,
    else (CPU, fp32 / fp64, a refusal) its torch twin ``<name>_reference``, counted as a fallback on a GPU."""
    from ...ops import transformer_native as TN
    if _native(like, "moe"):
        r = getattr(TN, name)(*args, **kw)
        if r is not None:
            return r
    if like.is_cuda:
        from ...ops import fallback
        fallback.record("moe", f"{name} dtype {like.dtype}: torch reference path")
    return getattr(TN, name + "_reference")(*args, **kw)


def _moe_bias(b):
    """An expert bias [X, N] as the grouped GEMM takes it: fp32 (fp64 stays fp64), contiguous."""
    if b.dtype in (torch.float32, torch.float64):
        return b.contiguous()
    return b.to(torch.float32).contiguous()


def _moe_grad(view, fn):
    """``fn(out)`` writes a per-expert gradient into ``out``: the gradient view itself when it is contiguous."""
    if view.is_contiguous():
        fn(view)
    else:
        tmp = torch.empty(view.shape, dtype=view.dtype, device=view.device)
        fn(tmp)
        copy_grad_(view, tmp)


def _add_into(a, b):
    """a + b written over b (the last residual add of a pre-norm block): the in-tree pairwise kernel on a GPU."""
    if a.is_cuda and ops.use_native(a, "rmsnorm"):
        from ...ops import nd4j_kernels
        if a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous() and \
                nd4j_kernels.binary(a, b, "add", out=b) is not None:
            return b
    return b.add_(a)


# ------------------------------------------------------------------------------------------------ dropout
class DropoutSites:
    """Dropout state of a transformer-family layer: ONE PhiloxStream per layer impl, advanced once per training
    forward (``dropoutBegin``); the layer's sites draw from streams with keys derived from the layer's seed that
    share its device counter, so their masks are independent and forward / backward of a step regenerate the same
    ones. Every mask taken OFF the kernels (CPU, fp32 / fp64, head sizes outside the flash kernel) comes from
    ``dropoutKeep``, which a test may override to feed the reference path another run's masks."""
    SITES = ("attention", "hidden1", "hidden2", "embedding")
    _drop_rng = None
    _drop_streams = None

    def dropoutBegin(self, device):
        from ...ops import nn_misc
        if self._drop_rng is None or self._drop_rng.offset.device != device:
            # the seed comes from torch's generator WITHOUT advancing it (a first training forward draws the same
            # reference-path masks as any later one under the same manual_seed); the layer's name and index make it
            # this layer's own
            import zlib
            with torch.random.fork_rng(devices=[]):
                base = nn_misc.PhiloxStream(device)
            name = str(getattr(self.conf, "layerName", None) or "")
            self._drop_rng = base.derive(len(self.SITES) + int(self.index or 0) + (zlib.crc32(name.encode()) << 8))
            self._drop_streams = {}
        self._drop_rng.advance()

    def dropoutStream(self, site):
        st = self._drop_streams.get(site)
        if st is None:
            st = self._drop_streams[site] = self._drop_rng.derive(self.SITES.index(site))
        return st

    def dropoutKeep(self, site, shape, drop, like):
        """Keep mask of ``shape`` for dropout site ``site``, already scaled by 1/keep (0 = dropped), on ``like``'s
        device: torch's generator and a saved mask, as nn/conf/regularization.py does on the CPU."""
        keep = 1.0 - drop
        return (torch.rand(tuple(shape), device=like.device, dtype=torch.float32) < keep).to(torch.float32) / keep


def _ln_fwd_drop(x, res, g, b, eps, drop, owner, site):
    """LN(drop(x) + res) -> (y, LayerNorm ctx, the x the LayerNorm backward takes, dropout ctx or None)."""
    if drop <= 0.0:
        y, ln = _ln_fwd(x, res, g, b, eps)
        return y, ln, x, None
    if _native(x, "layernorm"):
        from ...ops import transformer_native as TN
        if TN.ln_supported(x, x.shape[-1]):
            st = owner.dropoutStream(site)
            r = TN.ln_fwd_dropout(x, g, b, eps, res, drop, st, inplace=True)    # x: a GEMM output nobody else reads
            if r is not None:
                y, mean, rstd, xd = r
                return y, ("native", mean, rstd), xd, ("native", st, drop)
    keep = owner.dropoutKeep(site, x.shape, drop, x).to(x.dtype)
    xd = x * keep
    y, ln = _ln_fwd(xd, res, g, b, eps)
    return y, ln, xd, ("mask", keep)


def _drop_fwd(y, drop, owner, site):
    """drop(y) as its own launch (the embedding's dropout sits after its LayerNorm) -> (y', dropout ctx)."""
    from ...ops import nn_misc
    if y.is_cuda and y.is_contiguous() and nn_misc._dt(y) is not None and ops.use_native(y, "dropout"):
        st = owner.dropoutStream(site)
        return nn_misc.dropout_native(y, "dropout", st, False, p=1.0 - drop), ("native", st, drop)
    keep = owner.dropoutKeep(site, y.shape, drop, y).to(y.dtype)
    return y * keep, ("mask", keep)


def _drop_bwd(d, dctx):
    """d∘D for the mask of the forward (regenerated by the Philox kernel in backward mode, or the saved one)."""
    if dctx[0] == "native":
        from ...ops import nn_misc
        return nn_misc.dropout_native(d.contiguous(), "dropout", dctx[1], True, p=1.0 - dctx[2])
    return d * dctx[1].to(d.dtype)


# ------------------------------------------------------------------------------------------------ attention
def _attn_fwd(qkv, B, T, H, mask, causal, drop=0.0, owner=None, Hkv=None, window=None):
    from ...ops import transformer_native as TN
    Hkv = H if Hkv is None else Hkv
    if _native(qkv, "attention"):
        q3 = qkv.reshape(B, T, -1)
        if TN.attn_supported(q3, H, Hkv):
            if drop > 0.0:
                st = owner.dropoutStream("attention")
                out, lse = TN.attn_fwd(q3, H, mask, causal, dropout=drop, rng=st, Hkv=Hkv, window=window)
                return out.reshape(B * T, -1), ("native", out, lse, drop, st)
            out, lse = TN.attn_fwd(q3, H, mask, causal, Hkv=Hkv, window=window)
            return out.reshape(B * T, -1), ("native", out, lse)
    if qkv.is_cuda:
        from ...ops import fallback
        fallback.record("attention",
                        f"head size {qkv.shape[-1] // (H + 2 * Hkv)} / dtype {qkv.dtype}: explicit torch path")
    keep = owner.dropoutKeep("attention", (B, H, T, T), drop, qkv) if drop > 0.0 else None
    o, ctx = TN.attention_fwd_explicit(qkv.reshape(B, T, -1), H, mask, causal, keep=keep, Hkv=Hkv, window=window)
    return o.reshape(B * T, -1), ("explicit", ctx)


def _attn_bwd(dctx, qkv, B, T, H, mask, causal, ctx, Hkv=None, window=None):
    from ...ops import transformer_native as TN
    if ctx[0] == "native":
        kw = dict(dropout=ctx[3], rng=ctx[4]) if len(ctx) > 3 else {}
        return TN.attn_bwd(qkv.reshape(B, T, -1), ctx[1], ctx[2], dctx.reshape(B, T, -1), H, mask,
                           causal, Hkv=Hkv, window=window, **kw).reshape(B * T, -1)
    return TN.attention_bwd_explicit(ctx[1], dctx.reshape(B, T, -1), qkv.dtype).reshape(B * T, -1)


def _rope(qkv, B, T, H, Hkv, theta, what, inverse=False):
    """Rotary position embeddings on the Q | K columns of qkv [B*T, W] at positions 0 .. T-1 (``inverse``: the
    transposed rotation, for dQ | dK): csrc/attention_rope.hip in place on a GPU in bf16 / fp16 with head size
    64 / 128, else ``rope_reference``, counted as a fallback on a GPU. -> the rotated [B*T, W]."""
    from ...ops import transformer_native as TN
    q3 = qkv.reshape(B, T, -1)
    if _native(q3, "attention") and TN.attn_rope(q3, H, 0, theta, Hkv=Hkv, inverse=inverse) is not None:
        return qkv
    if qkv.is_cuda:
        from ...ops import fallback
        fallback.record("attention", f"{what} rotary embedding, head size {q3.shape[-1] // (H + 2 * Hkv)} / dtype "
                                     f"{qkv.dtype}: torch reference path")
    pos = torch.arange(T, device=qkv.device)
    return TN.rope_reference(q3, H, pos, theta, Hkv, inverse).reshape(qkv.shape)


# ------------------------------------------------------------------------------------------------ cached decoding
class KVCacheState:
    """rnnTimeStep state of a causal attention layer: one key/value cache ``kv [mb, Tcap, 2E]`` in the compute dtype
    (K of head h at column h*D, V at E + h*D; the layout of csrc/attention_decode.hip) and the number of valid rows.
    With grouped heads (``nKVHeads`` on the configuration) the cache holds the key/value heads only: 2*Ekv columns,
    or the fp8 rows of nKVHeads heads; everything below that moves whole rows does not care.
    Tcap is a multiple of 64 and grows geometrically, so a steady-state step neither allocates nor copies. The stored
    state handed out / taken in is ``{"kv": [mb, L, 2E]}`` trimmed to the valid length.

    Ragged batches: after a right-padded chunk ``rnnTrimState(lengths)`` stores ``short[b] = seen - lengths[b]``
    (int32 on the cache's device). ``_kv_len`` stays the upper bound the host counts; row b continues at
    ``_kv_len - short[b]``, overwriting what its padding left in the cache. The state then carries ``"short"``.

    ``cacheDataType="fp8"`` on the layer's configuration: the cache is uint8 ``[mb, Tcap, R]`` in the fp8 row format of
    csrc/attention_decode.hip (``ops.transformer_native.kv_fp8_row_bytes``), quantised by the append kernel and
    converted by the decode kernel as it stages; off the kernels the torch path stores and reads the same format.
    One tensor of 16-byte-multiple rows, so growth, trimming, reordering and pinning treat it as they treat the
    16-bit cache. A chunk of >= 64 tokens into an empty cache attends over its own unquantised K / V (the flash
    prompt path; only what it stores is quantised); every other chunk attends over what the cache holds, its own
    new rows included. The state handed out is ``{"kv": uint8 [mb, L, R], "kvFormat": "fp8"}``.

    A rotary layer (``positionEncoding="rotary"``) stores ROTATED keys: a token is rotated by the index of its cache
    row as it is appended. Everything that moves whole rows (growth, trimming, reordering, pinning, the cache format,
    the state handed out and taken in) needs nothing for that, but such a state is valid only for a layer with the
    same ``ropeTheta``."""
    _kv = None
    _kv_len = 0
    _kv_alt = None      # rnnReorderState's second buffer (same shape as _kv, or None): the two are swapped per call
    _kv_short = None    # int32 [mb] shortfall of every row against _kv_len (None: every row is _kv_len long)
    _kv_pinned = False  # rnnPinState: _kv_len is fixed at capacity - 1 and the network advances _kv_short on the device

    def rnnClearPreviousState(self):
        self._kv = self._kv_alt = self._kv_short = None
        self._kv_len = 0
        self._kv_pinned = False

    def rnnPinInfo(self):
        """What the network's rnnPinState reads: None (no cache, nothing to pin), or (tokens seen, mb, shortfall or
        None)."""
        return None if self._kv is None else (self._kv_len, self._kv.shape[0], self._kv_short)

    def rnnPinState(self, capacity, short, dryRun=False):
        """Pin the positions (the network's rnnPinState): the cache is reserved for ``capacity`` rows, the host bound
        becomes ``capacity - 1`` for good and ``short`` (int32 [mb] on the device, shared by every pinned layer of the
        network, which lowers it once per step) carries the rows' real positions: row b stands at
        ``capacity - 1 - short[b]``. ``dryRun`` only validates. A rotary layer's new token is rotated by that row
        index, read from ``short`` on the device."""
        if self._kv is None:
            return
        _pin_check(self, capacity, self._kv_len, self._kv_pinned)
        if dryRun:
            return
        mb, _, E2 = self._kv.shape
        self._kv_reserve(mb, E2, capacity, self._kv.dtype, self._kv.device)
        self._kv_len, self._kv_short, self._kv_pinned = int(capacity) - 1, short, True

    def rnnTrimState(self, lengths, dryRun=False):
        """The rows of the stored chunk(s) were right-padded: row b holds ``lengths[b]`` real tokens (1 <= lengths[b]
        <= tokens seen). ``lengths``: integers [mb] (read on the host once, here). Once per sequence; ``dryRun``
        only validates. A layer without a cache (a bidirectional block) has nothing to trim. A rotary layer's rows
        hold keys rotated by their own row index, which trimming does not change."""
        if self._kv is None:
            return
        _refuse_pinned(self, "rnnTrimState", self._kv_pinned)
        short = _trim_shortfall(self, lengths, self._kv_len, self._kv.shape[0], self._kv_short is not None)
        if not dryRun:
            self._kv_short = short.to(self._kv.device)

    def rnnSetPositions(self, bound, short, dryRun=False):
        """Set the rows' positions again (the network's rnnSetPositions): the host count becomes ``bound``
        (1 <= bound <= tokens seen) and ``short`` (int32 [mb], contiguous, on the cache's device; kept as it is, not
        copied, so a later in-place update on the device moves every layer that shares it) the shortfall: row b holds
        ``bound - short[b]`` tokens, and what the cache holds past that is overwritten by the next append. Any number
        of times per sequence, also after rnnTrimState; nothing is launched or read. The caller vouches for
        ``0 <= short[b] < bound`` (the kernels clamp). ``dryRun`` only validates. A layer without a cache has nothing
        to do. A rotary layer's surviving rows hold keys rotated by their own row index, which stays valid."""
        if self._kv is None:
            return
        _refuse_pinned(self, "rnnSetPositions", self._kv_pinned)
        _positions_check(self, bound, short, self._kv_len, self._kv.shape[0], self._kv.device)
        if not dryRun:
            self._kv_len, self._kv_short = int(bound), short

    def rnnReorderState(self, parents, groupSize=None):
        """Row i of the cache becomes the old row ``parents[i]`` (int32 device tensor [mbNew]; mbNew may differ from
        the stored minibatch size). The valid rows are gathered into a second buffer of the same capacity
        (csrc/generation.hip; never in place) and the two swap, so a steady-state call allocates nothing. Whole rows
        move and keep their row index, so a rotary layer's rotated keys stay valid."""
        kv = self._kv
        if kv is None:
            return
        _refuse_pinned(self, "rnnReorderState", self._kv_pinned)
        from ...ops import generation_native as GN
        shape = (int(parents.numel()), kv.shape[1], kv.shape[2])
        alt = self._kv_alt
        if alt is None or tuple(alt.shape) != shape or alt.dtype != kv.dtype or alt.device != kv.device:
            alt = torch.empty(shape, dtype=kv.dtype, device=kv.device)
        GN.cache_gather(kv, alt, parents, self._kv_len)
        self._kv_alt = kv if tuple(kv.shape) == shape else None
        self._kv = alt
        self._kv_short = _reorder_short(self._kv_short, parents, groupSize)

    def _kv_fp8(self):
        return getattr(self.conf, "cacheDataType", None) == "fp8"

    def _kv_heads(self):
        """The heads the cache holds: nKVHeads, or nHeads without grouping."""
        return getattr(self.conf, "nKVHeads", None) or self.conf.nHeads

    def rnnGetPreviousState(self):
        """The state of a rotary layer holds rotated keys: it is valid only for a layer with the same ``ropeTheta``."""
        if self._kv is None:
            return {}
        st = {"kv": self._kv[:, :self._kv_len].clone()}
        if self._kv.dtype == torch.uint8:
            st["kvFormat"] = "fp8"
        if self._kv_short is not None:
            st["short"] = self._kv_short.clone()
        return st

    def rnnSetPreviousState(self, state):
        """Takes the state in either format (16-bit / float ``kv [mb, L, 2E]``, or uint8 rows with
        ``"kvFormat": "fp8"``) and converts it to the layer's own (plain torch: not a hot path). A rotary layer takes
        the keys as rotated by a layer with its own ``ropeTheta``; nothing here can check that."""
        kv = state.get("kv") if state else None
        self.rnnClearPreviousState()
        if kv is None:
            return
        from ...ops import transformer_native as TN
        H = self._kv_heads()
        if state.get("kvFormat") == "fp8" and not self._kv_fp8():
            pad = -(-2 * H // 16) * 16
            kv = TN.kv_fp8_dequantize_reference(kv, H, (kv.shape[2] - pad) // (2 * H), self.compute_dtype)
        elif state.get("kvFormat") != "fp8" and self._kv_fp8():
            kv = TN.kv_fp8_quantize_reference(kv, H)
        mb, L, E2 = kv.shape
        self._kv_reserve(mb, E2, L, kv.dtype, kv.device)
        self._kv[:, :L] = kv
        self._kv_len = L
        if state.get("short") is not None:
            self._kv_short = _trim_shortfall(self, L - torch.as_tensor(state["short"]).cpu().to(torch.int64), L, mb,
                                             False).to(kv.device)

    def _check_state_mb(self, x):
        """rnnTimeStep continues the stored cache, so the minibatch size cannot change between calls without
        rnnClearPreviousState() (same rule and wording as BaseRecurrentImpl._check_state_mb)."""
        if self._kv is not None and self._kv.shape[0] != x.shape[0]:
            from ...exceptions import DL4JInvalidInputException
            raise DL4JInvalidInputException(
                f"rnnTimeStep on layer {self.index} ({type(self.conf).__name__}): minibatch size {x.shape[0]} differs "
                f"from the stored state's {self._kv.shape[0]}; call rnnClearPreviousState() before changing it")

    def _kv_reserve(self, mb, E2, need, dtype, device):
        """Make room for ``need`` rows: capacity is a multiple of 64 and at least doubles when it has to grow."""
        kv = self._kv
        if kv is not None and kv.shape[1] >= need and kv.dtype == dtype and kv.device == device:
            return
        cap = -(-max(int(need), 1) // 64) * 64
        if kv is not None:
            cap = max(cap, 2 * kv.shape[1])
        new = torch.empty(mb, cap, E2, dtype=dtype, device=device)
        if kv is not None and self._kv_len:
            new[:, :self._kv_len] = kv[:, :self._kv_len].to(dtype)
        self._kv = new
        self._kv_alt = None         # the second buffer follows the new capacity at the next rnnReorderState

    def cachedAttention(self, qkv, H, what="rnnTimeStep", Hkv=None, ropeTheta=None, window=None):
        """Causal attention of the chunk qkv [mb, Tn, 3E] ([mb, Tn, E + 2*Ekv] with ``Hkv`` key/value heads, which
        are what the cache then holds) over everything seen since rnnClearPreviousState(): its K / V
        are appended to the cache, its queries attend over the cache. -> [mb, Tn, E]. The decode kernels on a GPU in
        bf16 / fp16 with head size 64 / 128 (the causal flash forward for a prompt of >= 64 tokens into an empty
        cache), else the torch reference, counted as a fallback on a GPU. With the fp8 cache both paths store the
        quantised rows and attend over the dequantised cache, except for that prompt chunk.
        ``ropeTheta`` (a rotary layer): Q and K are rotated by their cache row index pos - short[b] + t, on the
        kernels by the append launch itself (``attn_rope_append``), so the cache holds rotated keys.
        ``window`` (the layer's ``attentionWindow``): a query at position p sees keys p - window < k <= p. The cache
        still keeps every row; the decode kernel skips the key blocks before the window, so a step reads
        O(window) rows whatever the cache holds."""
        from ...ops import transformer_native as TN
        mb, Tn, E3 = qkv.shape
        Hkv = H if Hkv is None else Hkv
        D = E3 // (H + 2 * Hkv)
        E, Ekv = H * D, Hkv * D
        pos, short = self._kv_len, self._kv_short
        if self._kv_pinned:
            _pinned_one_step(self, Tn)
        fp8 = self._kv_fp8()
        if fp8:
            self._kv_reserve(mb, TN.kv_fp8_row_bytes(Hkv, D), pos + Tn, torch.uint8, qkv.device)
        else:
            self._kv_reserve(mb, 2 * Ekv, pos + Tn, qkv.dtype, qkv.device)
        kv = self._kv
        out = done = None
        if _native(qkv, "attention") and qkv.is_contiguous() and TN.attn_decode_supported(qkv, kv, H, Hkv):
            done = TN.attn_kv_append(qkv, kv, H, pos, short, Hkv=Hkv) if ropeTheta is None else \
                TN.attn_rope_append(qkv, kv, H, pos, ropeTheta, short, Hkv=Hkv)
            if done is not None:
                if pos == 0 and Tn >= 64:
                    out = TN.attn_fwd(qkv, H, None, True, Hkv=Hkv, window=window)[0]
                else:
                    out = TN.attn_decode(qkv, kv, H, pos, short=short, Hkv=Hkv, window=window)
        if out is None:
            if qkv.is_cuda:
                from ...ops import fallback
                fallback.record("attention", f"{what} head size {E // H} / dtype {qkv.dtype}: torch reference path")
            if ropeTheta is not None and done is None:       # not rotated (and appended) by the kernel already
                qkv = TN.rope_reference(qkv, H, TN.rope_positions(mb, Tn, pos, short, qkv.device), ropeTheta, Hkv)
            new = TN.kv_fp8_quantize_reference(qkv[:, :, E:], Hkv) if fp8 else qkv[:, :, E:]
            if short is None:
                kv[:, pos:pos + Tn] = new
            else:
                rows = (pos - short.to(torch.int64)).reshape(mb, 1) + torch.arange(Tn, device=kv.device).reshape(1, Tn)
                kv[torch.arange(mb, device=kv.device).reshape(mb, 1), rows] = new
            if not fp8:
                seen = kv[:, :pos + Tn]
            elif pos == 0 and Tn >= 64:
                seen = qkv[:, :, E:]
            else:
                seen = TN.kv_fp8_dequantize_reference(kv[:, :pos + Tn], Hkv, D, qkv.dtype)
            out = TN.attention_decode_reference(qkv[:, :, :E], seen[:, :, :Ekv], seen[:, :, Ekv:], H, pos, short=short,
                                                Hkv=Hkv, window=window)
        if not self._kv_pinned:                  # pinned: the bound stays, the network lowers ``short`` on the device
            self._kv_len = pos + Tn
        return out


def _refuse_pinned(layer, what, pinned):
    if pinned:
        from ...exceptions import DL4JInvalidInputException
        raise DL4JInvalidInputException(
            f"{what} on layer {layer.index} ({type(layer.conf).__name__}): the state is pinned (rnnPinState), its "
            "positions advance on the device; call rnnClearPreviousState() first")


def _pinned_one_step(layer, Tn):
    if Tn != 1:
        from ...exceptions import DL4JInvalidInputException
        raise DL4JInvalidInputException(
            f"rnnTimeStep on layer {layer.index} ({type(layer.conf).__name__}): the state is pinned (rnnPinState) and "
            f"takes exactly one time step per call, got {Tn}")


def _pin_check(layer, capacity, seen, pinned, maxPositions=None):
    """A layer's validation of rnnPinState(capacity) with ``seen`` tokens stored."""
    from ...exceptions import DL4JInvalidInputException
    who = f"rnnPinState on layer {layer.index} ({type(layer.conf).__name__})"
    if pinned:
        raise DL4JInvalidInputException(
            f"{who}: the state is pinned already; call rnnClearPreviousState() to start a new sequence")
    if int(capacity) < seen + 1:
        raise DL4JInvalidInputException(
            f"{who}: capacity {capacity} leaves no room for a step after the {seen} tokens seen")
    if maxPositions is not None and int(capacity) > maxPositions:
        raise DL4JInvalidInputException(
            f"{who}: {seen} tokens seen + {int(capacity) - seen} new exceed maxPositions {maxPositions}; call "
            "rnnClearPreviousState() to start a new sequence")


def _trim_shortfall(layer, lengths, seen, mb, trimmed):
    """``seen - lengths`` as int32 [mb] on the host for a layer's rnnTrimState, after checking ``lengths`` (integers
    [mb], 1 <= lengths[b] <= seen) and that the state has not been trimmed already."""
    from ...exceptions import DL4JInvalidInputException
    who = f"rnnTrimState on layer {layer.index} ({type(layer.conf).__name__})"
    if trimmed:
        raise DL4JInvalidInputException(
            f"{who}: the state has been trimmed already; call rnnClearPreviousState() to start a new sequence")
    n = torch.as_tensor(lengths).detach().cpu().reshape(-1)
    if n.is_floating_point() or n.dtype == torch.bool or n.numel() != mb:
        raise DL4JInvalidInputException(
            f"{who}: lengths must be integers [{mb}] (one per row of the stored state), got {n.dtype} "
            f"{tuple(torch.as_tensor(lengths).shape)}")
    n = n.to(torch.int64)
    if n.numel() and (int(n.min()) < 1 or int(n.max()) > seen):
        raise DL4JInvalidInputException(
            f"{who}: every length must be in 1..{seen} (the tokens seen since rnnClearPreviousState()), got "
            f"{n.tolist()}")
    return (seen - n).to(torch.int32)


def _positions_check(layer, bound, short, seen, mb, device):
    """A layer's validation of rnnSetPositions(bound, short) with ``seen`` tokens stored in ``mb`` rows."""
    from ...exceptions import DL4JInvalidInputException
    who = f"rnnSetPositions on layer {layer.index} ({type(layer.conf).__name__})"
    if isinstance(bound, bool) or not isinstance(bound, int) or not 1 <= bound <= seen:
        raise DL4JInvalidInputException(
            f"{who}: bound must be an integer in 1..{seen} (the tokens seen since rnnClearPreviousState()), got "
            f"{bound!r}")
    if not (torch.is_tensor(short) and short.dtype == torch.int32 and tuple(short.shape) == (mb,) and
            short.is_contiguous()):
        got = f"{short.dtype} {tuple(short.shape)}" if torch.is_tensor(short) else type(short).__name__
        raise DL4JInvalidInputException(
            f"{who}: short must be a contiguous int32 tensor [{mb}] (one entry per row of the stored state), got "
            f"{got}")
    if short.device != device:
        raise DL4JInvalidInputException(f"{who}: short is on {short.device}, the stored state on {device}")


def _reorder_short(short, parents, groupSize):
    """rnnReorderState of a shortfall array: row i becomes the old row parents[i]. With ``groupSize`` and an unchanged
    number of rows nothing moves (the rows of a group share a prompt, so they share its length)."""
    if short is None or (groupSize is not None and short.shape[0] == parents.numel()):
        return short
    return short.index_select(0, parents.to(device=short.device, dtype=torch.int64)).contiguous()


def _token_major(x):
    """[mb, E, T] (possibly a permuted view of token-major memory) -> contiguous [mb*T, E] (no copy when it is)."""
    mb, E, T = x.shape
    return x.permute(0, 2, 1).reshape(mb * T, E)


class TransformerEncoderLayerImpl(KVCacheState, DropoutSites, LayerImpl):
    def type(self):
        return "RECURRENT"

    def activate(self, x, training=False, mask=None, **kw):
        c = self.conf
        if c.preNorm():
            return self._activate_pre(x, training, mask)
        self.training = training
        B, E, T = x.shape
        H = c.nHeads
        dt = self.W("Wqkv").dtype
        xt = _token_major(x).to(dt)
        m = mask.reshape(B, T) if mask is not None else None
        pa, ph = (float(c.attentionDropout), float(c.hiddenDropout)) if training else (0.0, 0.0)
        if pa > 0.0 or ph > 0.0:
            self.dropoutBegin(x.device)
        qkv = matmul(xt, self.W("Wqkv"), bias=self.Wbias("bqkv"))
        if c.rotary():                          # the rotated qkv is what the attention reads and backward keeps
            qkv = _rope(qkv, B, T, H, c.kvHeads(), c.ropeTheta, "TransformerEncoderLayer")
        ctx, actx = _attn_fwd(qkv, B, T, H, m, c.causal, pa, self, c.kvHeads(), c.attentionWindow)
        a = matmul(ctx, self.W("Wo"), bias=self.Wbias("bo"))
        h1, ln1, a, d1 = _ln_fwd_drop(a, xt, self.params["ln1g"], self.params["ln1b"], c.layerNormEps, ph, self,
                                      "hidden1")
        if c.nExperts is None:
            f, z1 = self._ffn1(h1, True)
            f2 = matmul(f, self.W("W2"), bias=self.Wbias("b2"))
        else:                                   # z1 carries the experts' context
            f, (f2, z1) = None, self._moe_fwd(h1)
        y, ln2, f2, d2 = _ln_fwd_drop(f2, h1, self.params["ln2g"], self.params["ln2b"], c.layerNormEps, ph, self,
                                      "hidden2")
        self.maskArray = mask
        if training:
            self._c = (xt, qkv, actx, ctx, a, ln1, h1, z1, f, f2, ln2, B, T, m, d1, d2)
        self.input = x
        return y.reshape(B, T, E).permute(0, 2, 1)

    def _ffn1(self, h, keep):
        """The first feed-forward projection and its activation -> (f, z1): GELU in the GEMM epilogue (z1, the
        pre-activation, kept for backward when ``keep``), or the fused gate | up projection z1 and ``swiglu``."""
        if self.conf.swiglu():
            z1 = matmul(h, self.W("W1"), bias=self.Wbias("b1"))
            return _swiglu_fwd(z1), z1
        if not keep:
            return matmul(h, self.W("W1"), bias=self.Wbias("b1"), act="gelu"), None
        # FFN-1 with bias + exact GELU fused into the GEMM epilogue; the pre-activation z1 is kept for backward
        z1 = torch.empty(h.shape[0], self.W("W1").shape[1], dtype=h.dtype, device=h.device)
        return matmul(h, self.W("W1"), bias=self.Wbias("b1"), act="gelu", z=z1), z1

    def _moe_fwd(self, n, acc=None):
        """The sparse feed-forward of n [N, E] -> (f2 [N, E] (+ ``acc``, written over it on the kernels), ctx =
        (plan, gate, Xp, Z1p, Fp, Yp) for ``_moe_bwd``)."""
        c = self.conf
        X, k, E = c.nExperts, c.nExpertsPerToken, n.shape[1]
        sixteen = n.dtype in (torch.bfloat16, torch.float16)
        logits = mmul(n, self.W("Wr"), out_dtype=torch.float32 if sixteen else None)
        plan, gate = _moe_op("moe_route", n, logits, k)
        W1, W2 = self.W("W1"), self.W("W2")
        xp = _moe_op("moe_gather", n, n, plan)
        z1p = _moe_op("gemm_grouped", n, xp, W1.view(X, E, -1), _moe_bias(self.Wbias("b1")), plan)
        fp = _swiglu_fwd(z1p) if c.swiglu() else _gelu_fwd(z1p)
        yp = _moe_op("gemm_grouped", n, fp, W2.view(X, -1, E), _moe_bias(self.Wbias("b2")), plan)
        if acc is not None and _native(n, "moe"):
            f2 = _moe_op("moe_combine", n, yp, plan, gate, acc, out=acc)
        else:
            f2 = _moe_op("moe_combine", n, yp, plan, gate, acc)
        return f2, (plan, gate, xp, z1p, fp, yp)

    def _moe_bwd(self, df2, n, ctx, acc=None):
        """-> dn, the gradient of the sparse feed-forward's input (+ ``acc``, the gradient arriving over the residual
        path, summed in place on the kernels); the gradients of Wr, W1, b1, W2, b2 land in their views."""
        from ...ops import transformer_native as TN
        c = self.conf
        X, E = c.nExperts, n.shape[1]
        plan, gate, xp, z1p, fp, yp = ctx
        g = self.grads
        df2 = df2.to(n.dtype).contiguous()
        W1, W2 = self.W("W1"), self.W("W2")
        dgate = _moe_op("moe_combine_bwd", n, df2, yp, plan)
        dyp = _moe_op("moe_gather", n, df2, plan, gate)
        _moe_grad(g["W2"], lambda out: _moe_op("gemm_grouped_wgrad", n, fp, dyp, plan, out))
        _moe_grad(g["b2"], lambda out: _moe_op("moe_segment_colsum", n, dyp, plan, out))
        dfp = _moe_op("gemm_grouped", n, dyp, W2.view(X, -1, E).transpose(1, 2), None, plan)
        dz1p = _swiglu_bwd(z1p, dfp) if c.swiglu() else _gelu_bwd(z1p, dfp)
        _moe_grad(g["W1"], lambda out: _moe_op("gemm_grouped_wgrad", n, xp, dz1p, plan, out))
        _moe_grad(g["b1"], lambda out: _moe_op("moe_segment_colsum", n, dz1p, plan, out))
        dxp = _moe_op("gemm_grouped", n, dz1p, W1.view(X, E, -1).transpose(1, 2), None, plan)
        if acc is not None and _native(n, "moe"):
            dn = _moe_op("moe_combine", n, dxp, plan, None, acc, out=acc)
        else:
            dn = _moe_op("moe_combine", n, dxp, plan, None, acc)
        dl = _moe_op("moe_route_bwd", n, plan, gate, dgate, n.dtype)
        _wgrad(g["Wr"], n, dl)
        return mmul(dl, self.W("Wr").t(), out=dn, beta=1.0)

    def _ffn1_bwd(self, df2, z1):
        """dz1, the gradient of the first projection's output, from df2, the gradient of the second's."""
        if self.conf.swiglu():
            return _swiglu_bwd(z1, matmul(df2, self.W("W2").t()))
        if _native(df2, "gemm") and z1.dtype == df2.dtype:
            # GELU backward in the GEMM epilogue: dz1 = (df2 · W2ᵀ) * gelu'(z1)
            return mmul(df2, self.W("W2").t(), act="dgelu", z=z1)
        return _gelu_bwd(z1, matmul(df2, self.W("W2").t()))

    def _activate_pre(self, x, training, mask):
        """The pre-norm block: h = x + drop(Attn(RMSNorm(x))), y = h + drop(FFN(RMSNorm(h))). The first residual add
        runs inside the second norm's launch (h overwrites the attention branch's output); the second is one launch
        of the pairwise kernel over the feed-forward branch's output."""
        c = self.conf
        self.training = training
        B, E, T = x.shape
        H = c.nHeads
        P = self.params
        xt = _token_major(x).to(self.W("Wqkv").dtype).contiguous()
        m = mask.reshape(B, T) if mask is not None else None
        pa, ph = (float(c.attentionDropout), float(c.hiddenDropout)) if training else (0.0, 0.0)
        if pa > 0.0 or ph > 0.0:
            self.dropoutBegin(x.device)
        n1, _, r1 = _rms_fwd(xt, None, P["ln1g"], c.layerNormEps)
        qkv = matmul(n1, self.W("Wqkv"), bias=self.Wbias("bqkv"))
        if c.rotary():
            qkv = _rope(qkv, B, T, H, c.kvHeads(), c.ropeTheta, "TransformerEncoderLayer")
        ctx, actx = _attn_fwd(qkv, B, T, H, m, c.causal, pa, self, c.kvHeads(), c.attentionWindow)
        a = matmul(ctx, self.W("Wo"), bias=self.Wbias("bo"))
        d1 = d2 = None
        if ph > 0.0:
            a, d1 = _drop_fwd(a, ph, self, "hidden1")
        n2, h, r2 = _rms_fwd(a, xt, P["ln2g"], c.layerNormEps, s_out=a)
        if c.nExperts is None:
            f, z1 = self._ffn1(n2, True)
            f2 = matmul(f, self.W("W2"), bias=self.Wbias("b2"))
        else:
            f, (f2, z1) = None, self._moe_fwd(n2)
        if ph > 0.0:
            f2, d2 = _drop_fwd(f2, ph, self, "hidden2")
        y = _add_into(h, f2)
        self.maskArray = mask
        if training:
            self._c = (xt, n1, r1, qkv, actx, ctx, h, n2, r2, z1, f, B, T, m, d1, d2)
        self.input = x
        return y.reshape(B, T, E).permute(0, 2, 1)

    def rnnTimeStep(self, x, mask=None):
        """One chunk [mb, E, Tn] (or one step [mb, E]) of a causal block continuing the cached keys / values: the
        inference forward of ``activate`` with the attention taken over the cache. A bidirectional block cannot
        stream and runs ``activate`` on the chunk."""
        c = self.conf
        if not c.causal:
            return self.activate(x, False, mask)
        self.training = False
        one = x.dim() == 2
        if one:
            x = x.unsqueeze(2)
        self._check_state_mb(x)
        B, E, T = x.shape
        xt = _token_major(x).to(self.W("Wqkv").dtype)
        if c.preNorm():
            xt = xt.contiguous()
            n1, _, _ = _rms_fwd(xt, None, self.params["ln1g"], c.layerNormEps)
            qkv = matmul(n1, self.W("Wqkv"), bias=self.Wbias("bqkv"))
        else:
            qkv = matmul(xt, self.W("Wqkv"), bias=self.Wbias("bqkv"))
        ctx = self.cachedAttention(qkv.reshape(B, T, -1), c.nHeads, Hkv=c.kvHeads(),
                                   ropeTheta=c.ropeTheta if c.rotary() else None,
                                   window=c.attentionWindow).reshape(B * T, -1)
        a = matmul(ctx, self.W("Wo"), bias=self.Wbias("bo"))
        if c.preNorm():
            n2, h, _ = _rms_fwd(a, xt, self.params["ln2g"], c.layerNormEps, s_out=a)
            if c.nExperts is not None:
                y = self._moe_fwd(n2, acc=h)[0]                 # y = h + f2: the add rides on the combine
                y = y.reshape(B, T, E).permute(0, 2, 1)
                return y[:, :, 0] if one else y
            f, _ = self._ffn1(n2, False)
            if _native(f, "gemm"):
                y = mmul(f, self.W("W2"), out=h, bias=bias_vec(self.Wbias("b2")), beta=1.0)   # y = h + f·W2 + b2
            else:
                y = _add_into(h, matmul(f, self.W("W2"), bias=self.Wbias("b2")))
        else:
            h1, _ = _ln_fwd(a, xt, self.params["ln1g"], self.params["ln1b"], c.layerNormEps)
            if c.nExperts is None:
                f, _ = self._ffn1(h1, False)
                f2 = matmul(f, self.W("W2"), bias=self.Wbias("b2"))
            else:
                f2 = self._moe_fwd(h1)[0]
            y, _ = _ln_fwd(f2, h1, self.params["ln2g"], self.params["ln2b"], c.layerNormEps)
        y = y.reshape(B, T, E).permute(0, 2, 1)
        return y[:, :, 0] if one else y

    def backpropGradient(self, eps, **kw):
        c = self.conf
        if c.preNorm():
            return self._backprop_pre(eps)
        xt, qkv, actx, ctx, a, ln1, h1, z1, f, f2, ln2, B, T, m, d1, d2 = self._c
        self._c = None
        g = self.grads
        dt = xt.dtype
        dy = _token_major(eps).to(dt)
        # ds2 / ds1: the residual's gradient. Without hidden dropout it is also the producing GEMM's (df2 / da) and its
        # column sums (b2 / bo gradient) come out of the LayerNorm backward launch; with it the producer's gradient is
        # ds∘D in a tensor of its own (ds stays the residual accumulator below) and the bias gradient ITS column sums.
        if d2 is None:
            ds2 = df2 = _ln_bwd(dy, f2, h1, self.params["ln2g"], ln2, g["ln2g"], g["ln2b"],
                                g["b2"] if c.nExperts is None else None)      # the experts' b2 [X, E]: _moe_bwd
        else:
            ds2 = _ln_bwd(dy, f2, h1, self.params["ln2g"], ln2, g["ln2g"], g["ln2b"])
            df2 = _drop_bwd(ds2, d2)
            if c.nExperts is None:
                _bsum(g["b2"], df2)
        if c.nExperts is None:
            _wgrad(g["W2"], f, df2)
            dz1 = self._ffn1_bwd(df2, z1)
            _wgrad(g["W1"], h1, dz1)
            _bsum(g["b1"], dz1)
            dh1 = mmul(dz1, self.W("W1").t(), out=ds2, beta=1.0)      # residual gradient summed in place
        else:
            dh1 = self._moe_bwd(df2, h1, z1, acc=ds2)
        if d1 is None:
            ds1 = da = _ln_bwd(dh1, a, xt, self.params["ln1g"], ln1, g["ln1g"], g["ln1b"], g["bo"])
        else:
            ds1 = _ln_bwd(dh1, a, xt, self.params["ln1g"], ln1, g["ln1g"], g["ln1b"])
            da = _drop_bwd(ds1, d1)
            _bsum(g["bo"], da)
        _wgrad(g["Wo"], ctx, da)
        dctx = matmul(da, self.W("Wo").t())
        dqkv = _attn_bwd(dctx, qkv, B, T, c.nHeads, m, c.causal, actx, c.kvHeads(), c.attentionWindow)
        if c.rotary():                          # the transposed rotation takes dQ | dK back to the projection's output
            dqkv = _rope(dqkv, B, T, c.nHeads, c.kvHeads(), c.ropeTheta, "TransformerEncoderLayer", inverse=True)
        _wgrad(g["Wqkv"], xt, dqkv)
        _bsum(g["bqkv"], dqkv)
        dx = mmul(dqkv, self.W("Wqkv").t(), out=ds1, beta=1.0)
        E = dx.shape[1]
        return self.make_gradient(), dx.reshape(B, T, E).permute(0, 2, 1)

    def _backprop_pre(self, eps):
        """The backward of ``_activate_pre``: dy flows to the feed-forward branch and, as ``dres`` of the second
        norm's backward, over the residual; dh likewise to the attention branch and into the first norm's backward,
        which adds it in place."""
        c = self.conf
        xt, n1, r1, qkv, actx, ctx, h, n2, r2, z1, f, B, T, m, d1, d2 = self._c
        self._c = None
        g = self.grads
        P = self.params
        dy = _token_major(eps).to(xt.dtype).contiguous()
        df2 = dy if d2 is None else _drop_bwd(dy, d2)
        if c.nExperts is None:
            _bsum(g["b2"], df2)
            _wgrad(g["W2"], f, df2)
            dz1 = self._ffn1_bwd(df2, z1)
            _wgrad(g["W1"], n2, dz1)
            _bsum(g["b1"], dz1)
            dn2 = matmul(dz1, self.W("W1").t())
        else:
            dn2 = self._moe_bwd(df2, n2, z1)
        # dh: the gradient of h = x + a. Without hidden dropout it is also the attention branch's (da) and its column
        # sums (bo's gradient) come out of the norm's backward launch
        if d1 is None:
            dh = da = _rms_bwd(dn2, h, P["ln2g"], r2, g["ln2g"], dres=dy, dsum_view=g["bo"])
        else:
            dh = _rms_bwd(dn2, h, P["ln2g"], r2, g["ln2g"], dres=dy)
            da = _drop_bwd(dh, d1)
            _bsum(g["bo"], da)
        _wgrad(g["Wo"], ctx, da)
        dctx = matmul(da, self.W("Wo").t())
        dqkv = _attn_bwd(dctx, qkv, B, T, c.nHeads, m, c.causal, actx, c.kvHeads(), c.attentionWindow)
        if c.rotary():
            dqkv = _rope(dqkv, B, T, c.nHeads, c.kvHeads(), c.ropeTheta, "TransformerEncoderLayer", inverse=True)
        _wgrad(g["Wqkv"], n1, dqkv)
        _bsum(g["bqkv"], dqkv)
        dn1 = matmul(dqkv, self.W("Wqkv").t())
        dx = _rms_bwd(dn1, xt, P["ln1g"], r1, g["ln1g"], dres=dh, dx_out=dh)
        E = dx.shape[1]
        return self.make_gradient(), dx.reshape(B, T, E).permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------ cross attention
def _cross_fwd(q, kv, B, Tq, Tk, H, kmask, what="cross attention"):
    """Attention of q [B*Tq, E] over rows [0, Tk) of kv [B, TkCap, 2E] (csrc/attention_cross.hip on a GPU in bf16 /
    fp16 with head size 64 / 128, else the explicit torch path, counted as a fallback on a GPU).
    -> (out [B*Tq, E], ctx for _cross_bwd)."""
    from ...ops import transformer_native as TN
    q3 = q.reshape(B, Tq, -1)
    if _native(q3, "attention") and TN.cross_attn_supported(q3, kv, H):
        r = TN.cross_attn_fwd(q3, kv, H, Tk, kmask)
        if r is not None:
            return r[0].reshape(B * Tq, -1), ("native", r[0], r[1])
    if q.is_cuda:
        from ...ops import fallback
        fallback.record("attention", f"{what} head size {q3.shape[-1] // H} / dtype {q.dtype}: explicit torch path")
    o, ctx = TN.cross_attention_fwd_explicit(q3, kv[:, :Tk], H, kmask)
    return o.reshape(B * Tq, -1), ("explicit", ctx)


def _cross_bwd(dctx, q, kv, B, Tq, Tk, H, kmask, ctx):
    """-> (dq [B*Tq, E], dkv [B*Tk, 2E])."""
    from ...ops import transformer_native as TN
    if ctx[0] == "native":
        dq, dkv = TN.cross_attn_bwd(q.reshape(B, Tq, -1), kv, ctx[1], ctx[2], dctx.reshape(B, Tq, -1), H, kmask, Tk=Tk)
    else:
        dq, dkv = TN.cross_attention_bwd_explicit(ctx[1], dctx.reshape(B, Tq, -1), q.dtype)
    return dq.reshape(B * Tq, -1), dkv.reshape(B * Tk, -1)


def _memory_mask(memoryMask, B, Tk):
    """The key-padding mask as the cross kernels take it: fp32 [B, Tk] contiguous, or None."""
    return None if memoryMask is None else memoryMask.reshape(B, Tk).to(torch.float32).contiguous()


class MemoryKVState:
    """rnnTimeStep state of a layer that attends over a memory: the memory's projection ``kv [mb, Tk, 2E]`` (the
    layout of csrc/attention_cross.hip) and its key-padding mask, computed on the first call after
    rnnClearPreviousState() that carries a memory and kept for the later steps, which pass ``memory=None``. Handed out
    / taken in as ``{"mem_kv": [mb, Tk, 2E], "mem_mask": [mb, Tk] or absent}``."""
    _mem_kv = None
    _mem_mask = None

    def memoryClear(self):
        self._mem_kv = self._mem_mask = None

    def memoryGet(self):
        if self._mem_kv is None:
            return {}
        st = {"mem_kv": self._mem_kv.clone()}
        if self._mem_mask is not None:
            st["mem_mask"] = self._mem_mask.clone()
        return st

    def memorySet(self, state):
        self.memoryClear()
        kv = state.get("mem_kv") if state else None
        if kv is None:
            return
        self._mem_kv = kv.contiguous().clone()
        m = state.get("mem_mask")
        self._mem_mask = None if m is None else _memory_mask(m, kv.shape[0], kv.shape[1]).clone()

    def memoryReorder(self, parents, groupSize=None):
        """Row i of the stored projection and mask becomes the old row ``parents[i]``. With ``groupSize`` the caller
        promises parents[i] // groupSize == i // groupSize over an unchanged number of rows: the rows of a group
        hold the same memory, so nothing moves."""
        kv = self._mem_kv
        if kv is None or (groupSize is not None and kv.shape[0] == parents.numel()):
            return
        from ...ops import generation_native as GN
        kv = kv.contiguous()
        new = torch.empty((int(parents.numel()),) + tuple(kv.shape[1:]), dtype=kv.dtype, device=kv.device)
        self._mem_kv = GN.cache_gather(kv, new, parents, kv.shape[1])
        if self._mem_mask is not None:
            self._mem_mask = self._mem_mask.index_select(0, parents.to(torch.int64)).contiguous()

    def memoryProject(self, x, memory, memoryMask, wkey, bkey):
        """The stored projection for a step on x [mb, E, Tn]: projected now when ``memory`` [mb, M, Tk] is given
        (one GEMM straight into the kv layout), else the one kept from an earlier call. -> (kv, Tk, mask)."""
        from ...exceptions import DL4JInvalidInputException
        who = f"rnnTimeStep on layer {self.index} ({type(self.conf).__name__})"
        if memory is not None:
            mb, M, Tk = memory.shape
            mt = _token_major(memory).to(self.W(wkey).dtype)
            self._mem_kv = matmul(mt, self.W(wkey), bias=self.Wbias(bkey)).reshape(mb, Tk, -1)
            self._mem_mask = _memory_mask(memoryMask, mb, Tk)
        elif self._mem_kv is None:
            raise DL4JInvalidInputException(
                f"{who}: no memory given and none stored; pass the memory on the first call after "
                "rnnClearPreviousState()")
        if self._mem_kv.shape[0] != x.shape[0]:
            raise DL4JInvalidInputException(
                f"{who}: minibatch size {x.shape[0]} differs from the stored memory's {self._mem_kv.shape[0]}; call "
                "rnnClearPreviousState() before changing it")
        return self._mem_kv, self._mem_kv.shape[1], self._mem_mask


class TransformerDecoderLayerImpl(MemoryKVState, KVCacheState, DropoutSites, LayerImpl):
    """Post-LN decoder block (conf: TransformerDecoderLayer), token-major like the encoder block:
      qkv = x·Wqkv + b;  h1 = LN(drop(causal_attention(qkv)·Wo + bo) + x)            self-attention (csrc/attention.hip)
      q2 = h1·Wq2 + b;  kv2 = mem·Wkv2 + b;  h2 = LN(drop(cross(q2, kv2)·Wo2 + bo2) + h1)   (csrc/attention_cross.hip)
      y  = LN(drop(gelu(h2·W1 + b1)·W2 + b2) + h2)
    The backward is written out by hand with the encoder block's pieces; it returns (dx, dmemory)."""
    SITES = DropoutSites.SITES + ("hidden3",)

    def type(self):
        return "RECURRENT"

    def activate(self, x, training=False, mask=None, memory=None, memoryMask=None, **kw):
        c = self.conf
        if memory is None:
            from ...exceptions import DL4JInvalidInputException
            raise DL4JInvalidInputException(
                f"layer {self.index} ({type(c).__name__}) takes two inputs: its own stream and a memory")
        self.training = training
        B, E, T = x.shape
        Tk = memory.shape[2]
        H = c.nHeads
        dt = self.W("Wqkv").dtype
        xt = _token_major(x).to(dt)
        mt = _token_major(memory).to(dt)
        m = mask.reshape(B, T) if mask is not None else None
        mm = _memory_mask(memoryMask, B, Tk)
        pa, ph = (float(c.attentionDropout), float(c.hiddenDropout)) if training else (0.0, 0.0)
        if pa > 0.0 or ph > 0.0:
            self.dropoutBegin(x.device)
        eps = c.layerNormEps
        P = self.params
        qkv = matmul(xt, self.W("Wqkv"), bias=self.Wbias("bqkv"))
        ctx1, actx = _attn_fwd(qkv, B, T, H, m, True, pa, self)
        a = matmul(ctx1, self.W("Wo"), bias=self.Wbias("bo"))
        h1, ln1, a, d1 = _ln_fwd_drop(a, xt, P["ln1g"], P["ln1b"], eps, ph, self, "hidden1")
        q2 = matmul(h1, self.W("Wq2"), bias=self.Wbias("bq2"))
        kv2 = matmul(mt, self.W("Wkv2"), bias=self.Wbias("bkv2")).reshape(B, Tk, -1)
        ctx2, cctx = _cross_fwd(q2, kv2, B, T, Tk, H, mm, "TransformerDecoderLayer")
        cc = matmul(ctx2, self.W("Wo2"), bias=self.Wbias("bo2"))
        h2, ln2, cc, d2 = _ln_fwd_drop(cc, h1, P["ln2g"], P["ln2b"], eps, ph, self, "hidden2")
        z1 = torch.empty(h2.shape[0], self.W("W1").shape[1], dtype=h2.dtype, device=h2.device)
        f = matmul(h2, self.W("W1"), bias=self.Wbias("b1"), act="gelu", z=z1)
        f2 = matmul(f, self.W("W2"), bias=self.Wbias("b2"))
        y, ln3, f2, d3 = _ln_fwd_drop(f2, h2, P["ln3g"], P["ln3b"], eps, ph, self, "hidden3")
        self.maskArray = mask
        if training:
            self._c = (xt, mt, qkv, actx, ctx1, a, ln1, h1, q2, kv2, cctx, ctx2, cc, ln2, h2, z1, f, f2, ln3, B, T, Tk,
                       m, mm, d1, d2, d3)
        self.input = x
        return y.reshape(B, T, E).permute(0, 2, 1)

    def backpropGradient(self, eps, **kw):
        c = self.conf
        (xt, mt, qkv, actx, ctx1, a, ln1, h1, q2, kv2, cctx, ctx2, cc, ln2, h2, z1, f, f2, ln3, B, T, Tk, m, mm, d1, d2,
         d3) = self._c
        self._c = None
        g = self.grads
        P = self.params
        H = c.nHeads
        dy = _token_major(eps).to(xt.dtype)

        def site(d, x, res, gk, bk, ln, bias, dctx):
            # (residual gradient, producer gradient): one tensor without hidden dropout, whose column sums (the
            # producer's bias gradient) come out of the LayerNorm backward launch; with it the producer's is ds∘D
            if dctx is None:
                ds = _ln_bwd(d, x, res, P[gk], ln, g[gk], g[bk], g[bias])
                return ds, ds
            ds = _ln_bwd(d, x, res, P[gk], ln, g[gk], g[bk])
            dp = _drop_bwd(ds, dctx)
            _bsum(g[bias], dp)
            return ds, dp

        ds3, df2 = site(dy, f2, h2, "ln3g", "ln3b", ln3, "b2", d3)
        _wgrad(g["W2"], f, df2)
        if _native(df2, "gemm") and z1.dtype == df2.dtype:
            dz1 = mmul(df2, self.W("W2").t(), act="dgelu", z=z1)
        else:
            dz1 = _gelu_bwd(z1, matmul(df2, self.W("W2").t()))
        _wgrad(g["W1"], h2, dz1)
        _bsum(g["b1"], dz1)
        dh2 = mmul(dz1, self.W("W1").t(), out=ds3, beta=1.0)          # residual gradient summed in place
        ds2, dcc = site(dh2, cc, h1, "ln2g", "ln2b", ln2, "bo2", d2)
        _wgrad(g["Wo2"], ctx2, dcc)
        dctx2 = matmul(dcc, self.W("Wo2").t())
        dq2, dkv2 = _cross_bwd(dctx2, q2, kv2, B, T, Tk, H, mm, cctx)
        _wgrad(g["Wq2"], h1, dq2)
        _bsum(g["bq2"], dq2)
        _wgrad(g["Wkv2"], mt, dkv2)
        _bsum(g["bkv2"], dkv2)
        dmem = matmul(dkv2, self.W("Wkv2").t())
        dh1 = mmul(dq2, self.W("Wq2").t(), out=ds2, beta=1.0)
        ds1, da = site(dh1, a, xt, "ln1g", "ln1b", ln1, "bo", d1)
        _wgrad(g["Wo"], ctx1, da)
        dctx1 = matmul(da, self.W("Wo").t())
        dqkv = _attn_bwd(dctx1, qkv, B, T, H, m, True, actx)
        _wgrad(g["Wqkv"], xt, dqkv)
        _bsum(g["bqkv"], dqkv)
        dx = mmul(dqkv, self.W("Wqkv").t(), out=ds1, beta=1.0)
        E = dx.shape[1]
        return self.make_gradient(), (dx.reshape(B, T, E).permute(0, 2, 1),
                                      dmem.reshape(B, Tk, -1).permute(0, 2, 1))

    def rnnTimeStep(self, x, mask=None, memory=None, memoryMask=None):
        """One chunk [mb, E, Tn] (or one step [mb, E]): the self-attention continues its key/value cache, the
        cross-attention runs the forward kernel (Tq = Tn) over the stored memory projection, which is computed when
        ``memory`` is given and reused while it is None."""
        c = self.conf
        self.training = False
        one = x.dim() == 2
        if one:
            x = x.unsqueeze(2)
        self._check_state_mb(x)
        B, E, T = x.shape
        H = c.nHeads
        P = self.params
        kv2, Tk, mm = self.memoryProject(x, memory, memoryMask, "Wkv2", "bkv2")
        xt = _token_major(x).to(self.W("Wqkv").dtype)
        qkv = matmul(xt, self.W("Wqkv"), bias=self.Wbias("bqkv"))
        ctx1 = self.cachedAttention(qkv.reshape(B, T, -1), H).reshape(B * T, -1)
        a = matmul(ctx1, self.W("Wo"), bias=self.Wbias("bo"))
        h1, _ = _ln_fwd(a, xt, P["ln1g"], P["ln1b"], c.layerNormEps)
        q2 = matmul(h1, self.W("Wq2"), bias=self.Wbias("bq2"))
        ctx2, _ = _cross_fwd(q2, kv2, B, T, Tk, H, mm, "TransformerDecoderLayer rnnTimeStep")
        cc = matmul(ctx2, self.W("Wo2"), bias=self.Wbias("bo2"))
        h2, _ = _ln_fwd(cc, h1, P["ln2g"], P["ln2b"], c.layerNormEps)
        f = matmul(h2, self.W("W1"), bias=self.Wbias("b1"), act="gelu")
        f2 = matmul(f, self.W("W2"), bias=self.Wbias("b2"))
        y, _ = _ln_fwd(f2, h2, P["ln3g"], P["ln3b"], c.layerNormEps)
        y = y.reshape(B, T, E).permute(0, 2, 1)
        return y[:, :, 0] if one else y

    def rnnClearPreviousState(self):
        KVCacheState.rnnClearPreviousState(self)
        self.memoryClear()

    def rnnReorderState(self, parents, groupSize=None):
        KVCacheState.rnnReorderState(self, parents, groupSize)
        self.memoryReorder(parents, groupSize)

    def rnnGetPreviousState(self):
        return dict(KVCacheState.rnnGetPreviousState(self), **self.memoryGet())

    def rnnSetPreviousState(self, state):
        KVCacheState.rnnSetPreviousState(self, state)
        self.memorySet(state)


class BertEmbeddingLayerImpl(DropoutSites, LayerImpl):
    def type(self):
        return "RECURRENT"

    def activate(self, x, training=False, mask=None, **kw):
        c = self.conf
        if x.dim() == 3:
            x = x[:, 0, :]
        idx = x.long()
        B, T = idx.shape
        dt = self.W("Wword").dtype
        from ...ops import nn_misc
        e = self._embed(idx, 0)
        y, ln = _ln_fwd(e, None, self.params["lng"], self.params["lnb"], c.layerNormEps)
        dctx = None
        if training and float(c.hiddenDropout) > 0.0:           # drop(LN(emb)): after the LayerNorm, its own launch
            self.dropoutBegin(y.device)
            y, dctx = _drop_fwd(y, float(c.hiddenDropout), self, "embedding")
        if training:
            self._c = (idx, e, ln, B, T, dctx)
        return y.reshape(B, T, -1).permute(0, 2, 1)

    def backpropGradient(self, eps, **kw):
        c = self.conf
        idx, e, ln, B, T, dctx = self._c
        self._c = None
        dy = _token_major(eps).to(e.dtype)
        if dctx is not None:
            dy = _drop_bwd(dy, dctx)
        g = self.grads
        de = _ln_bwd(dy, e, None, self.params["lng"], ln, g["lng"], g["lnb"])
        from ...ops import nd4j_kernels as NK
        from ...ops import nn_misc
        if de.is_cuda and g["Wword"].dtype == torch.float32:
            # word rows: scatter-add of the 16-bit row gradients into the fp32 view (in-tree kernel, no fp32 copy
            # of de); position / type rows: deterministic column sums written in place
            if getattr(self.net, "_grads_zeroed", False):
                nn_misc.embedding_backward_(g["Wword"], idx, de)     # flat gradient already cleared this step
            else:
                gw = NK.zero_(torch.empty_like(g["Wword"]))
                nn_misc.embedding_backward_(gw, idx, de)
                copy_grad_(g["Wword"], gw)
            # without a position table the position sums go to a scratch: the kernel pair still gives Wtype's row
            gpos = g["Wpos"] if c.positionEmbeddings else torch.empty(T, de.shape[1], dtype=torch.float32,
                                                                      device=de.device)
            if nn_misc.bert_embed_backward_pt(de.contiguous(), gpos, g["Wtype"], B, T):
                return self.make_gradient(), None
        de = de.to(g["Wword"].dtype)
        if getattr(self.net, "_grads_zeroed", False) and g["Wword"].is_contiguous():
            g["Wword"].index_add_(0, idx.reshape(-1), de)          # flat gradient already cleared this step
        else:
            gw = torch.zeros_like(g["Wword"])
            gw.index_add_(0, idx.reshape(-1), de)
            copy_grad_(g["Wword"], gw)
        if c.positionEmbeddings:
            copy_grad_(g["Wpos"][:T], de.reshape(B, T, -1).sum(0).to(g["Wpos"].dtype))
            if g["Wpos"].shape[0] > T:
                g["Wpos"][T:].zero_()
        gt = torch.zeros_like(g["Wtype"])
        gt[0] = de.sum(0)
        copy_grad_(g["Wtype"], gt)
        return self.make_gradient(), None

    def _embed(self, idx, pos, short=None):
        """[B*T, E] = Wword[idx] + Wpos[pos .. pos+T-1] + Wtype[0] in the compute dtype (in-tree kernel on a GPU);
        with ``short`` (int32 [B]) row b takes the positions from pos - short[b]. Without position embeddings
        (``positionEmbeddings(False)``) the Wpos addend is left out."""
        from ...ops import nn_misc
        B, T = idx.shape
        Wp = self.W("Wpos") if self.conf.positionEmbeddings else None
        e = nn_misc.bert_embed_forward(self.W("Wword"), Wp, self.W("Wtype"), idx, pos, short) \
            if idx.is_cuda else None
        if e is None:
            if Wp is None:
                wp = 0
            elif short is None:
                wp = self.W("Wpos")[pos:pos + T].repeat(B, 1)
            else:
                rows = (pos - short.to(torch.int64)).reshape(B, 1) + torch.arange(T, device=short.device).reshape(1, T)
                wp = self.W("Wpos")[rows.clamp(0, self.W("Wpos").shape[0] - 1).reshape(-1)]
            e = self.W("Wword")[idx.reshape(-1)] + wp + \
                self.W("Wtype")[0].reshape(1, -1)
            e = e.to(self.W("Wword").dtype).contiguous()
        return e

    # rnnTimeStep state: the number of tokens seen so far (and the minibatch size they were seen with); after
    # rnnTrimState the shortfall of every row against that count (int32 [mb] on the device), as in KVCacheState
    _seen = None
    _short = None
    _pinned = False     # rnnPinState: _seen stays (capacity - 1, mb) and the network advances _short on the device

    def rnnClearPreviousState(self):
        self._seen = self._short = None
        self._pinned = False

    def rnnPinInfo(self):
        return None if self._seen is None else (self._seen[0], self._seen[1], self._short)

    def rnnPinLimit(self):
        """The largest capacity rnnPinState takes: the position table's rows (None without one: no limit)."""
        return int(self.W("Wpos").shape[0]) if self.conf.positionEmbeddings else None

    def rnnPinState(self, capacity, short, dryRun=False):
        """Pin the positions as KVCacheState.rnnPinState does: the count of tokens seen becomes ``capacity - 1`` for
        good and row b's next token takes position ``capacity - 1 - short[b]``. ``capacity`` beyond maxPositions is
        refused here, once, instead of at the step that would reach it."""
        if self._seen is None:
            return
        _pin_check(self, capacity, self._seen[0], self._pinned,
                   self.W("Wpos").shape[0] if self.conf.positionEmbeddings else None)
        if not dryRun:
            self._seen, self._short, self._pinned = (int(capacity) - 1, self._seen[1]), short, True

    def rnnTrimState(self, lengths, dryRun=False):
        """Row b of what has been fed so far holds ``lengths[b]`` real tokens, right-padded: its next token takes
        position ``lengths[b]``. Validated on the host, once per sequence; ``dryRun`` only validates."""
        _refuse_pinned(self, "rnnTrimState", self._pinned)
        pos, mb = self._seen if self._seen is not None else (0, torch.as_tensor(lengths).numel())
        short = _trim_shortfall(self, lengths, pos, mb, self._short is not None)
        if not dryRun:
            self._short = short.to(self.params["Wword"].device)

    def rnnSetPositions(self, bound, short, dryRun=False):
        """Set the rows' positions again, as KVCacheState.rnnSetPositions: the count of tokens seen becomes ``bound``
        and row b's next token takes position ``bound - short[b]``; ``short`` is kept as it is, not copied."""
        if self._seen is None:
            return
        _refuse_pinned(self, "rnnSetPositions", self._pinned)
        _positions_check(self, bound, short, self._seen[0], self._seen[1], self.params["Wword"].device)
        if not dryRun:
            self._seen, self._short = (int(bound), self._seen[1]), short

    def rnnReorderState(self, parents, groupSize=None):
        if self._seen is not None:
            _refuse_pinned(self, "rnnReorderState", self._pinned)
            self._seen = (self._seen[0], int(parents.numel()))
            self._short = _reorder_short(self._short, parents, groupSize)

    def rnnGetPreviousState(self):
        if self._seen is None:
            return {}
        st = {"pos": self._seen[0], "mb": self._seen[1]}
        if self._short is not None:
            st["short"] = self._short.clone()
        return st

    def rnnSetPreviousState(self, state):
        self.rnnClearPreviousState()
        if state and "pos" in state:
            self._seen = (int(state["pos"]), int(state["mb"]))
            if state.get("short") is not None:
                n = self._seen[0] - torch.as_tensor(state["short"]).cpu().to(torch.int64)
                self._short = _trim_shortfall(self, n, self._seen[0], self._seen[1], False) \
                    .to(self.params["Wword"].device)

    def rnnTimeStep(self, x, mask=None):
        """Token ids [mb, Tn] (or [mb, 1, Tn]) embedded at positions pos .. pos+Tn-1, pos = the tokens seen since
        rnnClearPreviousState()."""
        from ...exceptions import DL4JInvalidInputException
        if x.dim() == 3:
            x = x[:, 0, :]
        idx = x.long()
        B, T = idx.shape
        pos, mb = self._seen if self._seen is not None else (0, B)
        if mb != B:
            raise DL4JInvalidInputException(
                f"rnnTimeStep on layer {self.index} ({type(self.conf).__name__}): minibatch size {B} differs "
                f"from the stored state's {mb}; call rnnClearPreviousState() before changing it")
        if self._pinned:
            _pinned_one_step(self, T)
        maxp = self.W("Wpos").shape[0] if self.conf.positionEmbeddings else None
        if maxp is not None and pos + T > maxp:
            raise DL4JInvalidInputException(
                f"rnnTimeStep on layer {self.index} ({type(self.conf).__name__}): {pos} tokens seen + {T} new exceed "
                f"maxPositions {maxp}; call rnnClearPreviousState() to start a new sequence")
        self.training = False
        e = self._embed(idx, pos, self._short)
        y, _ = _ln_fwd(e, None, self.params["lng"], self.params["lnb"], self.conf.layerNormEps)
        if not self._pinned:
            self._seen = (pos + T, B)
        return y.reshape(B, T, -1).permute(0, 2, 1)

    def feedForwardMaskArray(self, mask, state, mb):
        self.maskArray = mask
        return mask, state


class BertPoolerLayerImpl(LayerImpl):
    def activate(self, x, training=False, mask=None, **kw):
        from ...ops import nd4j_kernels as NK
        self.input = x
        x0 = x[:, :, 0].to(self.W("W").dtype)
        if training and x0.is_cuda:
            # keep the pre-activation: backward is eps * tanh'(z) on the in-tree derivative kernel (the GEMM
            # epilogue stores a pre-activation for GELU only)
            z = matmul(x0, self.W("W"), bias=self.Wbias("b"))
            y = NK.transform(z, "tanh")
            if y is not None:
                self._c = (x0, z, None, x.shape)
                return y
            y = torch.tanh(z)
        else:
            y = matmul(x0, self.W("W"), bias=self.Wbias("b"), act="tanh")
        if training:
            self._c = (x0, None, y, x.shape)
        return y

    def backpropGradient(self, eps, **kw):
        from ...ops import nd4j_kernels as NK
        x0, z, y, shape = self._c
        self._c = None
        dz = NK.transform_bp(z, eps.to(z.dtype), "tanh") if z is not None else None
        if dz is None:
            y = torch.tanh(z) if y is None else y
            dz = eps.to(y.dtype) * (1 - y * y)
        _wgrad(self.grads["W"], x0, dz)
        _bsum(self.grads["b"], dz)
        B, E, T = shape
        if x0.is_cuda:
            # token-major [B, T, E] storage returned as a [B, E, T] view, so the encoder below reads it without a
            # transposing copy; only token 0 receives a gradient
            dxt = NK.zero_(torch.empty((B, T, E), dtype=x0.dtype, device=x0.device))
            mmul(dz, self.W("W").t(), out=dxt[:, 0, :])
            return self.make_gradient(), dxt.permute(0, 2, 1)
        dx = torch.zeros(shape, dtype=x0.dtype, device=x0.device)
        dx[:, :, 0] = matmul(dz, self.W("W").t())
        return self.make_gradient(), dx

    def feedForwardMaskArray(self, mask, state, mb):
        return None, state
