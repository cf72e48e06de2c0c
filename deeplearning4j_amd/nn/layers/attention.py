"""Multi-head self-attention over recurrent-format activations [mb, nIn, T].

Not in the reference snapshot (no attention/LayerNorm layers exist there); added for the
transformer configs the rebuild targets. Everything runs on the in-tree kernels with a
hand-derived backward (no torch.autograd):

  forward   X = x^T [mb*T, nIn];  QKV = X [Wq|Wk|Wv] + [bq|bk|bv]  (three GEMMs writing the column blocks of one
            [mb*T, 3d] buffer, bias in the epilogue);  O = attention(QKV)  (flash kernel csrc/attention.hip for
            bf16 / fp16 with head size 64 / 128, else the explicit reference, counted as a fallback on the GPU);
            Y = O Wo + bo;  masked query rows zeroed;  y = act(Y^T)
  backward  dY = act'(.) eps (masked rows zeroed);  dWo = O^T dY, dbo = colsum(dY);  dO = dY Wo^T;
            dQKV = attention_bwd(dO) (flash backward kernel, or P-based explicit backward);
            dW{q,k,v} = X^T dQ/dK/dV, db{q,k,v} = colsums;  dX = dQ Wq^T + dK Wk^T + dV Wv^T (beta-accumulated GEMMs)
Feature masks [mb, T] mask padded keys; masked query rows produce zeros.
``attentionDropout`` (a DROP probability, training only): the keep mask is generated inside the flash kernels from
the layer's PhiloxStream and regenerated in the backward; the explicit path takes its mask from ``dropoutKeep``.
``nKVHeads`` (grouped-query attention): Wk / Wv project to the nKVHeads key/value heads only, the buffer is
[mb*T, d + 2*dkv] (Q | K | V, dkv = nKVHeads * headSize), the kernels share each key/value head between the
nHeads / nKVHeads query heads of its group and dK / dV come back summed over the group.
``rnnTimeStep`` on a causal layer appends the chunk's K / V to a per-layer cache and attends over it
(``KVCacheState`` in transformer.py, csrc/attention_decode.hip).
``positionEncoding="rotary"``: the Q and K columns of the buffer are rotated by their positions after the projection
(csrc/attention_rope.hip, in place), the rotated buffer is what the attention reads and the backward keeps, and the
transposed rotation is applied to dQ | dK before the weight, bias and input gradients.

``CrossAttentionLayerImpl`` is the two-sequence counterpart (a two-input graph layer): Q = X Wq + bq from its own
stream [mb, nIn, Tq], KV = M Wkv + bkv from the memory [mb, nInMemory, Tk] in one GEMM straight into the
kv [mb, Tk, 2d] layout of csrc/attention_cross.hip; backward dWo, dbo, dO = dY Wo^T, (dQ, dKV) from the cross
backward kernels, dWq / dWkv and their biases, dX = dQ Wq^T, dM = dKV Wkv^T, returned as the pair (dX, dM).
"""
import torch

from .base import LayerImpl, bias_grad_, matmul, weight_grad_
from .transformer import DropoutSites, KVCacheState, MemoryKVState, _cross_bwd, _cross_fwd, _memory_mask, _rope
from ...ops.gemm import mmul


class SelfAttentionLayerImpl(KVCacheState, DropoutSites, LayerImpl):
    def type(self):
        return "RECURRENT"

    def _dims(self):
        c = self.conf
        hs = c.headSize or (c.nOut // c.nHeads)
        return c.nHeads, hs, c.nHeads * hs

    def _kv_dims(self):
        """(key/value heads, dkv = their columns, the column blocks of Q | K | V in the fused buffer)."""
        H, hs, d = self._dims()
        Hkv = self.conf.kvHeads()
        dkv = Hkv * hs
        return Hkv, dkv, ((0, d), (d, d + dkv), (d + dkv, d + 2 * dkv))

    def _project(self, X, n, device):
        """QKV [n, d + 2*dkv]: three GEMMs writing the column blocks of one buffer, bias in the epilogue."""
        _, dkv, blocks = self._kv_dims()
        qkv = torch.empty(n, blocks[2][1], dtype=X.dtype, device=device)
        for (lo, hi), (wk, bk) in zip(blocks, (("Wq", "bq"), ("Wk", "bk"), ("Wv", "bv"))):
            mmul(X, self.W(wk), out=qkv[:, lo:hi], bias=self.Wbias(bk).reshape(-1))
        return qkv

    def _attn_fwd(self, qkv, mb, T, H, mask, drop=0.0):
        from ...ops import transformer_native as TN
        from ...ops import use_native
        q3 = qkv.reshape(mb, T, -1)
        Hkv = self.conf.kvHeads()
        if q3.is_cuda and q3.dtype in (torch.bfloat16, torch.float16) and use_native(q3, "attention") \
                and TN.attn_supported(q3, H, Hkv):
            if drop > 0.0:
                st = self.dropoutStream("attention")
                out, lse = TN.attn_fwd(q3, H, mask, bool(self.conf.causal), dropout=drop, rng=st, Hkv=Hkv,
                                       window=self.conf.attentionWindow)
                return out, ("native", out, lse, drop, st)
            out, lse = TN.attn_fwd(q3, H, mask, bool(self.conf.causal), Hkv=Hkv, window=self.conf.attentionWindow)
            return out, ("native", out, lse)
        if q3.is_cuda:
            from ...ops import fallback
            fallback.record("attention", f"SelfAttentionLayer head size {q3.shape[-1] // (H + 2 * Hkv)} / {q3.dtype}")
        keep = self.dropoutKeep("attention", (mb, H, T, T), drop, q3) if drop > 0.0 else None
        out, ctx = TN.attention_fwd_explicit(q3, H, mask, bool(self.conf.causal), keep=keep, Hkv=Hkv,
                                             window=self.conf.attentionWindow)
        return out, ("explicit", ctx)

    def _attn_bwd(self, qkv, do, mb, T, H, mask, ctx):
        from ...ops import transformer_native as TN
        if ctx[0] == "native":
            kw = dict(dropout=ctx[3], rng=ctx[4]) if len(ctx) > 3 else {}
            return TN.attn_bwd(qkv.reshape(mb, T, -1), ctx[1], ctx[2], do.reshape(mb, T, -1), H, mask,
                               bool(self.conf.causal), Hkv=self.conf.kvHeads(), window=self.conf.attentionWindow,
                               **kw)
        return TN.attention_bwd_explicit(ctx[1], do.reshape(mb, T, -1), qkv.dtype)

    def activate(self, x, training=False, mask=None, **kw):
        self.training = training
        mb, nIn, T = x.shape
        H, hs, d = self._dims()
        dt = self.W("Wq").dtype
        X = x.permute(0, 2, 1).reshape(mb * T, nIn).to(dt).contiguous()
        qkv = self._project(X, mb * T, x.device)
        if self.conf.rotary():
            qkv = _rope(qkv, mb, T, H, self.conf.kvHeads(), self.conf.ropeTheta, "SelfAttentionLayer")
        m = mask.reshape(mb, T) if mask is not None else None
        drop = float(self.conf.attentionDropout) if training else 0.0
        if drop > 0.0:
            self.dropoutBegin(x.device)
        o, actx = self._attn_fwd(qkv, mb, T, H, m, drop)
        o2 = o.reshape(mb * T, d)
        Y = matmul(o2, self.W("Wo"), bias=self.Wbias("bo"))
        if m is not None:
            Y = Y * m.reshape(mb * T, 1).to(Y.dtype)
        z = Y.reshape(mb, T, -1).permute(0, 2, 1)
        self.input = x
        self.maskArray = mask
        if training:
            self._c = (X, qkv, actx, o2, m, mb, T)
        self._z = z
        return self.conf.activation.getActivation(z, training) if self.conf.activation is not None else z

    def rnnTimeStep(self, x, mask=None):
        """One chunk [mb, nIn, Tn] (or one step [mb, nIn]) of a causal layer continuing the cached keys / values; a
        bidirectional layer cannot stream and runs ``activate`` on the chunk."""
        if not self.conf.causal:
            return self.activate(x, False)
        self.training = False
        one = x.dim() == 2
        if one:
            x = x.unsqueeze(2)
        self._check_state_mb(x)
        mb, nIn, T = x.shape
        H, hs, d = self._dims()
        dt = self.W("Wq").dtype
        X = x.permute(0, 2, 1).reshape(mb * T, nIn).to(dt).contiguous()
        qkv = self._project(X, mb * T, x.device)
        o = self.cachedAttention(qkv.reshape(mb, T, -1), H, "SelfAttentionLayer rnnTimeStep", self.conf.kvHeads(),
                                 self.conf.ropeTheta if self.conf.rotary() else None, self.conf.attentionWindow)
        Y = matmul(o.reshape(mb * T, d), self.W("Wo"), bias=self.Wbias("bo"))
        z = Y.reshape(mb, T, -1).permute(0, 2, 1)
        y = self.conf.activation.getActivation(z, False) if self.conf.activation is not None else z
        return y[:, :, 0] if one else y

    def backpropGradient(self, eps, **kw):
        X, qkv, actx, o2, m, mb, T = self._c
        H, hs, d = self._dims()
        dz = self.conf.activation.backprop(self._z, eps.to(self._z.dtype)) if self.conf.activation is not None \
            else eps
        dt = X.dtype
        dY = dz.permute(0, 2, 1).reshape(mb * T, -1).to(dt)
        if m is not None:
            dY = dY * m.reshape(mb * T, 1).to(dt)
        dY = dY.contiguous()
        weight_grad_(self.grads["Wo"], o2.t(), dY)
        bias_grad_(self.grads["bo"], dY)
        dO = matmul(dY, self.W("Wo").t())
        blocks = self._kv_dims()[2]
        dqkv = self._attn_bwd(qkv, dO, mb, T, H, m, actx).reshape(mb * T, blocks[2][1])
        if not dqkv.is_contiguous():
            dqkv = dqkv.contiguous()
        if self.conf.rotary():
            dqkv = _rope(dqkv, mb, T, H, self.conf.kvHeads(), self.conf.ropeTheta, "SelfAttentionLayer", inverse=True)
        Xt = X.t()
        dX = None
        for (lo, hi), (wk, bk) in zip(blocks, (("Wq", "bq"), ("Wk", "bk"), ("Wv", "bv"))):
            g = dqkv[:, lo:hi]
            weight_grad_(self.grads[wk], Xt, g)
            bias_grad_(self.grads[bk], g.contiguous() if g.is_cuda else g)
            if dX is None:
                dX = mmul(g, self.W(wk).t())
            else:
                mmul(g, self.W(wk).t(), out=dX, beta=1.0)
        self._c = None
        eps_prev = dX.reshape(mb, T, -1).permute(0, 2, 1)
        return self.make_gradient(), eps_prev


class CrossAttentionLayerImpl(MemoryKVState, LayerImpl):
    def type(self):
        return "RECURRENT"

    def _dims(self):
        c = self.conf
        hs = c.headSize or (c.nOut // c.nHeads)
        return c.nHeads, hs, c.nHeads * hs

    def _forward(self, X, kv, mb, T, Tk, mm, m, what):
        H, hs, d = self._dims()
        q = matmul(X, self.W("Wq"), bias=self.Wbias("bq"))
        o2, cctx = _cross_fwd(q, kv, mb, T, Tk, H, mm, what)
        Y = matmul(o2, self.W("Wo"), bias=self.Wbias("bo"))
        if m is not None:
            Y = Y * m.reshape(mb * T, 1).to(Y.dtype)
        return q, o2, cctx, Y.reshape(mb, T, -1).permute(0, 2, 1)

    def activate(self, x, training=False, mask=None, memory=None, memoryMask=None, **kw):
        if memory is None:
            from ...exceptions import DL4JInvalidInputException
            raise DL4JInvalidInputException(
                f"layer {self.index} ({type(self.conf).__name__}) takes two inputs: its own stream and a memory")
        self.training = training
        mb, nIn, T = x.shape
        Tk = memory.shape[2]
        dt = self.W("Wq").dtype
        X = x.permute(0, 2, 1).reshape(mb * T, nIn).to(dt).contiguous()
        M = memory.permute(0, 2, 1).reshape(mb * Tk, memory.shape[1]).to(dt).contiguous()
        kv = matmul(M, self.W("Wkv"), bias=self.Wbias("bkv")).reshape(mb, Tk, -1)
        m = mask.reshape(mb, T) if mask is not None else None
        mm = _memory_mask(memoryMask, mb, Tk)
        q, o2, cctx, z = self._forward(X, kv, mb, T, Tk, mm, m, "CrossAttentionLayer")
        self.input = x
        self.maskArray = mask
        if training:
            self._c = (X, M, q, kv, cctx, o2, m, mm, mb, T, Tk)
        self._z = z
        return self.conf.activation.getActivation(z, training) if self.conf.activation is not None else z

    def backpropGradient(self, eps, **kw):
        X, M, q, kv, cctx, o2, m, mm, mb, T, Tk = self._c
        self._c = None
        H, hs, d = self._dims()
        dz = self.conf.activation.backprop(self._z, eps.to(self._z.dtype)) if self.conf.activation is not None \
            else eps
        dt = X.dtype
        dY = dz.permute(0, 2, 1).reshape(mb * T, -1).to(dt)
        if m is not None:
            dY = dY * m.reshape(mb * T, 1).to(dt)
        dY = dY.contiguous()
        weight_grad_(self.grads["Wo"], o2.t(), dY)
        bias_grad_(self.grads["bo"], dY)
        dO = matmul(dY, self.W("Wo").t())
        dq, dkv = _cross_bwd(dO, q, kv, mb, T, Tk, H, mm, cctx)
        weight_grad_(self.grads["Wq"], X.t(), dq)
        bias_grad_(self.grads["bq"], dq)
        weight_grad_(self.grads["Wkv"], M.t(), dkv)
        bias_grad_(self.grads["bkv"], dkv)
        dX = matmul(dq, self.W("Wq").t())
        dM = matmul(dkv, self.W("Wkv").t())
        return self.make_gradient(), (dX.reshape(mb, T, -1).permute(0, 2, 1), dM.reshape(mb, Tk, -1).permute(0, 2, 1))

    def rnnTimeStep(self, x, mask=None, memory=None, memoryMask=None):
        """One chunk [mb, nIn, Tn] (or one step [mb, nIn]) attending over the stored memory projection, which is
        computed when ``memory`` is given and reused while it is None."""
        self.training = False
        one = x.dim() == 2
        if one:
            x = x.unsqueeze(2)
        mb, nIn, T = x.shape
        kv, Tk, mm = self.memoryProject(x, memory, memoryMask, "Wkv", "bkv")
        X = x.permute(0, 2, 1).reshape(mb * T, nIn).to(self.W("Wq").dtype).contiguous()
        m = mask.reshape(mb, T) if mask is not None else None
        z = self._forward(X, kv, mb, T, Tk, mm, m, "CrossAttentionLayer rnnTimeStep")[3]
        y = self.conf.activation.getActivation(z, False) if self.conf.activation is not None else z
        return y[:, :, 0] if one else y

    def rnnClearPreviousState(self):
        self.memoryClear()

    def rnnReorderState(self, parents, groupSize=None):
        self.memoryReorder(parents, groupSize)

    def rnnTrimState(self, lengths, dryRun=False):
        """The stored memory projection does not depend on how long the rows of the own stream are: nothing to do."""

    def rnnSetPositions(self, bound, short, dryRun=False):
        """The stored memory projection has no position of the own stream: nothing to do."""

    def rnnPinInfo(self):
        """The stored memory projection has no position that advances: nothing to pin."""
        return None

    def rnnPinState(self, capacity, short, dryRun=False):
        pass

    def rnnGetPreviousState(self):
        return self.memoryGet()

    def rnnSetPreviousState(self, state):
        self.memorySet(state)
