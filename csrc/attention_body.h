// The flash-attention kernel bodies for gfx950, shared by self attention (csrc/attention.hip) and cross attention
// (csrc/attention_cross.hip): bf16 or fp16 in (template element type hb) / fp32 accumulate, head dim D in {64, 128}.
// The __global__ kernels of those files only say where their operands live and call a body; a numerics or tuning
// change is made here, once. Cached decoding (csrc/attention_decode.hip) has the forward wave mapping and per-block
// arithmetic in a kernel of its own and shares the host-side helpers at the end of this file.
//
// Operands are plain pointers and strides (in elements), E = H*D, head h at column h*D of its row:
//   Q      qp + b*q_bs + row*q_ld            (qkv[B,T,3E]: q_bs = T*3E, q_ld = 3E;  q[B,Tq,E]: Tq*E, E)
//   K      kp + b*k_bs + row*k_ld, V at K + E (qkv: kp = qkv + E;  kv[B,TkCap,2E]: k_bs = TkCap*2E, k_ld = 2E)
//   dQ / dK likewise, dV at dK + E;  out, dout [B,Tq,E];  mask [B,Tk] fp32 (1 = keep) or null;  lse, dq_dot [B,H,Tq].
// Query rows are bounded by Tq and key rows by Tk, never one by the other; self attention passes Tq = Tk = T.
//
// Grouped-query attention (the GQA = true instances of the three bodies; csrc/attention.hip has the layouts): H query
// heads share Hkv = H / G key/value heads, query head h uses kv head h / G. K of kv head j sits at kp + j*D and V
// v_off elements after it (an operand, Ekv = Hkv*D in a cache, the same in the fused projection); dK likewise, dV at
// dK + v_off. lse, dq_dot and the dropout mask stay indexed by the QUERY head. With GQA = false G is the constant 1
// and v_off the constant E: those instances are the kernels as they were, not a run-time special case.
//
// Sliding window (the WIN = true instances of the three bodies, causal only): query q sees keys q - window < k <= q.
// The forward and dQ bodies start at the first key block the tile's first query sees, max(0, q0 - window + 1) / BLK
// (for NB = 2 a round may therefore start at an odd block: rounds carry no alignment), the dK/dV body stops at the last
// query block that sees its key block, and the score mask gains key > q - window. Blocks outside are skipped, not
// masked; the dropout tile stays keyed by the absolute (q, k), so a pair keeps its draw with and without a window.
// With WIN and DROP the dQ body computes Delta itself in a first pass over its blocks (see there) and the dK/dV
// kernel, launched after it, reads that. With WIN = false the bodies are the kernels as they were.
//
// CDNA4 mapping (per 64-wide wave, v_mfma_f32_16x16x32_{bf16,f16}):
//  * forward / dQ: grid (ceil(Tq/64), B*H); a wave owns 16 queries. Scores are computed TRANSPOSED, Sᵀ = K·Qᵀ, so the
//    query is the lane's accumulator column: the online-softmax state (running max m, sum l) is one scalar per lane and
//    the 64 keys of a block reduce with two cross-group shuffles. Pᵀ stays in registers and feeds Oᵀ += Vᵀ·Pᵀ directly as
//    the B operand (the k-slot order of the accumulator layout is matched on the A side by reading Vᵀ from LDS in the
//    same permuted key order), so P never touches LDS.
//  * dK/dV: grid (ceil(Tk/64), B*H); a wave owns 16 keys; S = Q·Kᵀ has the key on the lane; dVᵀ += dOᵀ·P and
//    dKᵀ += Qᵀ·dS take P / dS as B operands the same way. dQ is a separate pass over query blocks (no atomics, so
//    results are bitwise reproducible).
//  * K/V (or Q/dO) tiles are staged in LDS per 64-row block, both row-major and transposed as the operands need;
//    rows padded by 16 B.
// Softmax runs in the exp2 domain: s2 = q·k · scale·log2(e); lse2 = m2 + log2(l) is saved for the backward. A query
// with no visible key gives zero output and the 1e30 lse sentinel, so every backward probability is
// exp2(s - 1e30) = 0 and its gradients are zero.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "attention_mma.h"

// ------------------------------------------------------------------------------------------------ dropout mask
// Attention-probability dropout (DROP = true instances of the bodies below; the DROP = false instances are the kernels
// without it, no run-time branch). The keep mask is never stored: it is a pure function of
// (seed, offset, b*H + h, q, k), independent of tiling, NB, head size and kernel, regenerated in the backward.
//   * one Philox-4x32-10 call covers the 4x4 (q, k) tile: counter {k >> 2, q >> 2, b*H + h, low 32 bits of offset},
//     key {seed low, seed high};
//   * element (q & 3, k & 3) is byte (k & 3) of result word (q & 3); it is kept iff byte >= thr, thr = round(drop*256);
//   * kept probabilities are rescaled by 1 / keep_eff, keep_eff = 1 - thr/256 (the rate actually drawn).
// A lane of the forward / dQ bodies holds one query x 4 consecutive keys per 16x16 accumulator tile (one word, four
// bytes), a lane of the dK/dV body one key x 4 consecutive queries (one byte of each word): one call per lane per
// tile in all three. offset is read from device memory (the layer's step counter), so graph replays draw new masks.
// ops/transformer_native.py::attn_dropout_keep is the host oracle of this mapping.
struct DropArgs {
  unsigned long long seed = 0;
  const long long* offset = nullptr;
  unsigned thr = 0;
  float inv_keep = 1.f;
};
__device__ __forceinline__ uint4 attn_drop_tile(unsigned long long seed, unsigned off, unsigned bh, unsigned q4,
                                                unsigned k4) {
  return philox4x32_10(make_uint4(k4, q4, bh, off), make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
}
__device__ __forceinline__ unsigned attn_drop_word(const uint4& t, int qi) {
  return qi == 0 ? t.x : (qi == 1 ? t.y : (qi == 2 ? t.z : t.w));
}
__device__ __forceinline__ bool attn_drop_keep(unsigned word, int ki, unsigned thr) {
  return ((word >> (8 * ki)) & 0xffu) >= thr;
}

// ------------------------------------------------------------------------------------------------ inner step
// the D columns of one row as A/B fragments (16-byte pieces at 32*ks + 8*hgrp)
template <int D, typename hb>
__device__ __forceinline__ void attn_ld_frag(V8<hb> (&f)[D / 32], const hb* row, int hgrp) {
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) f[ks] = ld8(row + ks * 32 + 8 * hgrp);
}

// one 16x16 tile of rows·fᵀ: rows [16*mt, 16*mt + 16) of a staged 64-row block (row stride D + 8) against the
// fragments f of the lane's own row
template <int D, typename hb>
__device__ __forceinline__ f4_t attn_score_tile(const hb* rows, const V8<hb> (&f)[D / 32], int mt, int col, int hgrp) {
  f4_t s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) s = mma(ld8(rows + (mt * 16 + col) * (D + 8) + ks * 32 + 8 * hgrp), f[ks], s);
  return s;
}
// the scores of one 64-key block: s[mt][r] = k[16*mt + 4*hgrp + r] · q
template <int D, typename hb>
__device__ __forceinline__ void attn_scores(f4_t (&s)[4], const hb* Kj, const V8<hb> (&qf)[D / 32], int col, int hgrp) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) s[mt] = attn_score_tile<D>(Kj, qf, mt, col, hgrp);
}

// accᵀ += Vᵀ·Pᵀ over 32 rows of a 64-row block: pb = pack2 of their two probability tiles, Vth = their columns of a
// transposed tile (row stride ldv). The callers pack one half at a time, right before its products: the forward
// kernels' register count depends on that order.
template <int D, typename hb>
__device__ __forceinline__ void attn_pv_half(f4_t (&acc)[D / 16], V8<hb> pb, const hb* Vth, int ldv, int col,
                                             int hgrp) {
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) acc[dt] = mma(ld4x2(Vth + (dt * 16 + col) * ldv, hgrp), pb, acc[dt]);
}

// the lane's 4 x D/16 accumulator values times mul, rounded to hb, into its row (D columns at row)
template <int D, typename hb>
__device__ __forceinline__ void attn_store_tile(hb* row, const f4_t (&acc)[D / 16], float mul, int hgrp) {
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const V4<hb> v{tobf<hb>(acc[dt][0] * mul), tobf<hb>(acc[dt][1] * mul), tobf<hb>(acc[dt][2] * mul),
                   tobf<hb>(acc[dt][3] * mul)};
    *reinterpret_cast<V4<hb>*>(row + dt * 16 + hgrp * 4) = v;
  }
}

// One 64-row block of K and V (V at K + v_off), D/32 16-byte chunks of each per thread of a 256-thread block: first
// into registers (rows at or beyond `rows` read as zeros), then K row-major into Kj and V transposed into Vtj, so a
// caller can keep the loads of one block in flight while it works on another.
template <int D, typename hb>
__device__ __forceinline__ void attn_kv_fetch(V8<hb> (&kr)[D / 32], V8<hb> (&vr)[D / 32], const hb* kbase,
                                              long long k_ld, int v_off, int row0, int rows) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int it = 0; it < D / 32; ++it) {
    const int i = threadIdx.x + it * 256, r = i / CPR, c = i - r * CPR;
    const bool ok = row0 + r < rows;
    const hb* src = kbase + (long long)(ok ? row0 + r : 0) * k_ld + c * 8;
    kr[it] = ok ? ld8(src) : V8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
    vr[it] = ok ? ld8(src + v_off) : V8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
  }
}
template <int D, typename hb>
__device__ __forceinline__ void attn_kv_stash(hb* Kj, hb* Vtj, int ldv, const V8<hb> (&kr)[D / 32],
                                              const V8<hb> (&vr)[D / 32]) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int it = 0; it < D / 32; ++it) {
    const int i = threadIdx.x + it * 256, r = i / CPR, c = i - r * CPR;
    *reinterpret_cast<V8<hb>*>(Kj + r * (D + 8) + c * 8) = kr[it];
#pragma unroll
    for (int k = 0; k < 8; ++k) Vtj[(c * 8 + k) * ldv + r] = vr[it][k];
  }
}

// ------------------------------------------------------------------------------------------------ forward
// NB key blocks are staged per round (NB = 2 for D = 64: a Tk = 128 sequence is one round, one global round trip and
// one barrier pair instead of two); every thread issues all of the round's K and V loads before any LDS store.
// DROP: O = (P o D) V with the running max / sum and lse from the undropped scores (lse is that of the DROP = false
// instance); dropped probabilities are zeroed before the PV product and 1/keep_eff is folded into the final 1/l.
// The masking and online-softmax update is written out here: as a helper function it is optimised on its own before
// it is inlined, its exp2 / add order changes, and the D = 64 instances go from 116-124 to 132-136 VGPRs, one wave per
// SIMD less.
template <int D, typename hb, int NB, bool DROP, bool GQA = false, bool WIN = false>
__device__ __forceinline__ void attn_fwd_body(const hb* qp, long long q_bs, long long q_ld, const hb* kp,
                                              long long k_bs, long long k_ld, const float* mask, hb* out, float* lse,
                                              int Tq, int Tk, int H, float scale2, int causal, DropArgs da,
                                              int Garg = 1, int v_off_arg = 0, int window = 0) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDK = D + 8, LDV = NB * BLK + 8;
  __shared__ __attribute__((aligned(16))) hb Ks[NB * BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Vt[D * LDV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int E = H * D;
  const int v_off = GQA ? v_off_arg : E;
  const hb* kbase = kp + (long long)b * k_bs + (GQA ? h / Garg : h) * D;
  const int q = blockIdx.x * BLK + wave * 16 + col;
  const int qc = min(q, Tq - 1);
  V8<hb> qf[KS];
  attn_ld_frag<D>(qf, qp + (long long)b * q_bs + (long long)qc * q_ld + h * D, hgrp);
  f4_t acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  float m = kNegInf, l = 0.f;
  unsigned drop_off = 0;
  if constexpr (DROP) drop_off = (unsigned)da.offset[0];
  const float* mrow = mask ? mask + (long long)b * Tk : nullptr;
  const int nkb = causal ? min((blockIdx.x * BLK + BLK + BLK - 1) / BLK, (Tk + BLK - 1) / BLK) : (Tk + BLK - 1) / BLK;
  const int rows = min(Tk, nkb * BLK);                           // blocks at or beyond nkb are not loaded
  int kb_first = 0;                                              // WIN: the first block the tile's first query sees
  if constexpr (WIN) kb_first = max(0, (int)blockIdx.x * BLK - window + 1) / BLK;
  for (int kb0 = kb_first; kb0 < nkb; kb0 += NB) {
    __syncthreads();
    V8<hb> kr[NB][KS], vr[NB][KS];
#pragma unroll
    for (int j = 0; j < NB; ++j) attn_kv_fetch<D>(kr[j], vr[j], kbase, k_ld, v_off, (kb0 + j) * BLK, rows);
#pragma unroll
    for (int j = 0; j < NB; ++j) attn_kv_stash<D>(Ks + j * BLK * LDK, Vt + j * BLK, LDV, kr[j], vr[j]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int kb = kb0 + j;
      if (kb >= nkb) break;
      f4_t s[4];
      attn_scores<D>(s, Ks + j * BLK * LDK, qf, col, hgrp);
      float bm = kNegInf;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb * BLK + mt * 16 + hgrp * 4 + r;
          bool ok = key < Tk && (!causal || key <= q);
          if constexpr (WIN) ok = ok && key > q - window;
          if (ok && mrow) ok = mrow[key] != 0.f;
          const float v = ok ? s[mt][r] * scale2 : kNegInf;
          s[mt][r] = v;
          bm = fmaxf(bm, v);
        }
      bm = wmax16(bm);
      const float mn = fmaxf(m, bm);
      const float alpha = (mn == kNegInf) ? 1.f : exp2f(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = (mn == kNegInf) ? 0.f : exp2f(s[mt][r] - mn);
          s[mt][r] = p;
          ps += p;
        }
      l = l * alpha + wsum16(ps);
      m = mn;
      if constexpr (DROP) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const unsigned w = attn_drop_word(
              attn_drop_tile(da.seed, drop_off, (unsigned)bh, (unsigned)q >> 2, (unsigned)(kb * 16 + mt * 4 + hgrp)),
              q & 3);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (!attn_drop_keep(w, r, da.thr)) s[mt][r] = 0.f;
        }
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2)
        attn_pv_half<D>(acc, pack2<hb>(s[2 * k2], s[2 * k2 + 1]), Vt + j * BLK + 32 * k2, LDV, col, hgrp);
    }
  }
  if (q < Tq) {
    float inv = l > 0.f ? 1.f / l : 0.f;
    if constexpr (DROP) inv *= da.inv_keep;
    attn_store_tile<D>(out + ((long long)b * Tq + q) * E + h * D, acc, inv, hgrp);
    if (hgrp == 0) lse[(long long)bh * Tq + q] = l > 0.f ? m + log2f(l) : 1e30f;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// Dq[b,h,q] = sum_d dO[q,d] * O[q,d]; o and dout [B,T,H*D]
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_bwd_pre_kernel(const hb* __restrict__ o, const hb* __restrict__ dout,
                                                           float* __restrict__ dq_dot, int B, int T, int H) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over B*H*T
  if (i >= (long long)B * H * T) return;
  const int q = (int)(i % T);
  const long long bh = i / T;
  const int h = (int)(bh % H), b = (int)(bh / H);
  const long long off = ((long long)b * T + q) * H * D + h * D;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    const V8<hb> a = ld8(o + off + c * 8), g = ld8(dout + off + c * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (float)a[k] * (float)g[k];
  }
  dq_dot[i] = s;
}

// dQ per query block (forward orientation: query on the lane). DROP: dS = P o (D o dP - Delta), D in {0, 1/keep_eff}.
template <int D, typename hb, bool DROP, bool GQA = false, bool WIN = false>
__device__ __forceinline__ void attn_bwd_dq_body(const hb* qp, long long q_bs, long long q_ld, const hb* kp,
                                                 long long k_bs, long long k_ld, const hb* dout, const float* mask,
                                                 const float* lse, const float* dq_dot, hb* dq, long long dq_bs,
                                                 long long dq_ld, int Tq, int Tk, int H, float scale2, float scale,
                                                 int causal, DropArgs da, int Garg = 1, int v_off_arg = 0,
                                                 int window = 0, float* delta_out = nullptr) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDK = D + 8, LDT = BLK + 8;
  __shared__ __attribute__((aligned(16))) hb Ks[BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Vs[BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Kt[D * LDT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int E = H * D;
  const int v_off = GQA ? v_off_arg : E;
  const hb* kbase = kp + (long long)b * k_bs + (GQA ? h / Garg : h) * D;
  const int q = blockIdx.x * BLK + wave * 16 + col;
  const int qc = min(q, Tq - 1);
  V8<hb> qf[KS], df[KS];
  attn_ld_frag<D>(qf, qp + (long long)b * q_bs + (long long)qc * q_ld + h * D, hgrp);
  attn_ld_frag<D>(df, dout + ((long long)b * Tq + qc) * E + h * D, hgrp);
  const float l2 = lse[(long long)bh * Tq + qc];
  float dd = 0.f;
  if constexpr (!(WIN && DROP)) dd = dq_dot[(long long)bh * Tq + qc];
  unsigned drop_off = 0;
  if constexpr (DROP) drop_off = (unsigned)da.offset[0];
  f4_t acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  const float* mrow = mask ? mask + (long long)b * Tk : nullptr;
  const int nkb = causal ? min((blockIdx.x * BLK + BLK + BLK - 1) / BLK, (Tk + BLK - 1) / BLK) : (Tk + BLK - 1) / BLK;
  int kb_first = 0;                                              // WIN: as in the forward
  if constexpr (WIN) kb_first = max(0, (int)blockIdx.x * BLK - window + 1) / BLK;
  if constexpr (WIN && DROP) {
    // Delta = sum_k P (D o dP) over the window's few blocks, in fp32 from this pass's own probabilities, instead of
    // dO . O from the stored output: O = (P o D) V / keep_eff is rounded to 16 bits, and where a query sees few keys
    // dS = P (D o dP - Delta) cancels down to that rounding (with one visible key the exact dS is zero). A first
    // pass over the same blocks in the same order; the result also goes to delta_out for the dK/dV kernel, which
    // is launched after this one. No atomics: the sum runs in a fixed order.
    float part = 0.f;
    for (int kb = kb_first; kb < nkb; ++kb) {
      __syncthreads();
      stage_rows<D>(Ks, LDK, kbase, k_ld, kb * BLK, Tk);
      stage_rows<D>(Vs, LDK, kbase + v_off, k_ld, kb * BLK, Tk);
      __syncthreads();
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const f4_t s = attn_score_tile<D>(Ks, qf, mt, col, hgrp), dp = attn_score_tile<D>(Vs, df, mt, col, hgrp);
        const unsigned w = attn_drop_word(
            attn_drop_tile(da.seed, drop_off, (unsigned)bh, (unsigned)q >> 2, (unsigned)(kb * 16 + mt * 4 + hgrp)),
            q & 3);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb * BLK + mt * 16 + hgrp * 4 + r;
          bool ok = key < Tk && q < Tq && key <= q && key > q - window && attn_drop_keep(w, r, da.thr);
          if (ok && mrow) ok = mrow[key] != 0.f;
          if (ok) part += exp2f(s[r] * scale2 - l2) * (dp[r] * da.inv_keep);
        }
      }
    }
    dd = wsum16(part);
    if (hgrp == 0 && q < Tq) delta_out[(long long)bh * Tq + q] = dd;
  }
  for (int kb = kb_first; kb < nkb; ++kb) {
    __syncthreads();
    stage_rows<D>(Ks, LDK, kbase, k_ld, kb * BLK, Tk);
    stage_rows<D>(Vs, LDK, kbase + v_off, k_ld, kb * BLK, Tk);
    stage_rows_t<D>(Kt, LDT, kbase, k_ld, kb * BLK, Tk);
    __syncthreads();
    f4_t s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = attn_score_tile<D>(Ks, qf, mt, col, hgrp);
      dp[mt] = attn_score_tile<D>(Vs, df, mt, col, hgrp);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      unsigned w = 0;
      if constexpr (DROP)
        w = attn_drop_word(
            attn_drop_tile(da.seed, drop_off, (unsigned)bh, (unsigned)q >> 2, (unsigned)(kb * 16 + mt * 4 + hgrp)),
            q & 3);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb * BLK + mt * 16 + hgrp * 4 + r;
        bool ok = key < Tk && q < Tq && (!causal || key <= q);
        if constexpr (WIN) ok = ok && key > q - window;
        if (ok && mrow) ok = mrow[key] != 0.f;
        const float p = ok ? exp2f(s[mt][r] * scale2 - l2) : 0.f;
        float dpv = dp[mt][r];
        if constexpr (DROP) dpv = attn_drop_keep(w, r, da.thr) ? dpv * da.inv_keep : 0.f;
        s[mt][r] = p * (dpv - dd);                               // dS (w.r.t. the scaled scores)
      }
    }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)                               // dQᵀ += Kᵀ·dSᵀ
      attn_pv_half<D>(acc, pack2<hb>(s[2 * k2], s[2 * k2 + 1]), Kt + 32 * k2, LDT, col, hgrp);
  }
  if (q < Tq) attn_store_tile<D>(dq + (long long)b * dq_bs + (long long)q * dq_ld + h * D, acc, scale, hgrp);
}

// dK, dV per key block (key on the lane), looping over the query blocks of Tq. DROP: dV = (P o D)^T dO (dropped P
// zeroed, 1/keep_eff folded into the final store), dS as in the dQ body.
// GQA: grid.y is B*Hkv; the block loads its K / V fragments once and runs the query-block loop for each query head
// g = 0 .. G-1 of its group in that fixed order (that head's Q, dO, lse, dq_dot and dropout tile), dK and dV
// accumulating in the same fp32 registers and stored once: no atomics, no workspace, bitwise reproducible.
template <int D, typename hb, bool DROP, bool GQA = false, bool WIN = false>
__device__ __forceinline__ void attn_bwd_dkdv_body(const hb* qp, long long q_bs, long long q_ld, const hb* kp,
                                                   long long k_bs, long long k_ld, const hb* dout, const float* mask,
                                                   const float* lse, const float* dq_dot, hb* dk_out, long long dk_bs,
                                                   long long dk_ld, int Tq, int Tk, int H, float scale2, float scale,
                                                   int causal, DropArgs da, int Garg = 1, int v_off_arg = 0,
                                                   int window = 0) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDQ = D + 8, LDT = BLK + 8;
  __shared__ __attribute__((aligned(16))) hb Qs[BLK * LDQ];
  __shared__ __attribute__((aligned(16))) hb Ds[BLK * LDQ];
  __shared__ __attribute__((aligned(16))) hb Qt[D * LDT];
  __shared__ __attribute__((aligned(16))) hb Dt[D * LDT];
  __shared__ float Ls[BLK], Dd[BLK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int G = GQA ? Garg : 1, Hkv = GQA ? H / G : H;
  const int bj = blockIdx.y, b = bj / Hkv, j = bj - b * Hkv;   // kv head j; without GQA it is the query head
  const int E = H * D;
  const int v_off = GQA ? v_off_arg : E;
  const int key = blockIdx.x * BLK + wave * 16 + col;
  const int kc = min(key, Tk - 1);
  unsigned drop_off = 0;
  if constexpr (DROP) drop_off = (unsigned)da.offset[0];
  bool kvalid = key < Tk;
  if (kvalid && mask) kvalid = mask[(long long)b * Tk + key] != 0.f;
  V8<hb> kf[KS], vf[KS];
  const hb* krow = kp + (long long)b * k_bs + (long long)kc * k_ld + j * D;
  attn_ld_frag<D>(kf, krow, hgrp);
  attn_ld_frag<D>(vf, krow + v_off, hgrp);
  f4_t dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  int nqb = (Tq + BLK - 1) / BLK;
  // WIN: the last query that sees a key of this block is its last key + window - 1 (the host keeps window <= Tq)
  if constexpr (WIN) nqb = min(nqb, ((int)blockIdx.x * BLK + BLK - 1 + window - 1) / BLK + 1);
  const int qb0 = causal ? blockIdx.x : 0;                     // queries before the key block see none of it
  for (int g = 0; g < G; ++g) {
    const int h = GQA ? j * G + g : j;
    const int bh = GQA ? b * H + h : bj;
    const hb* qbase = qp + (long long)b * q_bs + h * D;
    const hb* dbase = dout + (long long)b * Tq * E + h * D;
    for (int qb = qb0; qb < nqb; ++qb) {
      __syncthreads();
      stage_rows<D>(Qs, LDQ, qbase, q_ld, qb * BLK, Tq);
      stage_rows<D>(Ds, LDQ, dbase, E, qb * BLK, Tq);
      stage_rows_t<D>(Qt, LDT, qbase, q_ld, qb * BLK, Tq);
      stage_rows_t<D>(Dt, LDT, dbase, E, qb * BLK, Tq);
      if (threadIdx.x < BLK) {
        const int qq = min(qb * BLK + (int)threadIdx.x, Tq - 1);
        Ls[threadIdx.x] = lse[(long long)bh * Tq + qq];
        Dd[threadIdx.x] = dq_dot[(long long)bh * Tq + qq];
      }
      __syncthreads();
      f4_t s[4], dp[4], ds[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        s[mt] = attn_score_tile<D>(Qs, kf, mt, col, hgrp);
        dp[mt] = attn_score_tile<D>(Ds, vf, mt, col, hgrp);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        uint4 dtile = make_uint4(0, 0, 0, 0);
        if constexpr (DROP)
          dtile = attn_drop_tile(da.seed, drop_off, (unsigned)bh, (unsigned)(qb * 16 + mt * 4 + hgrp),
                                 (unsigned)key >> 2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = mt * 16 + hgrp * 4 + r, q = qb * BLK + qi;
          bool ok = kvalid && q < Tq && (!causal || key <= q);
          if constexpr (WIN) ok = ok && key > q - window;
          const float p = ok ? exp2f(s[mt][r] * scale2 - Ls[qi]) : 0.f;
          float dpv = dp[mt][r];
          bool keep = true;
          if constexpr (DROP) {
            keep = attn_drop_keep(attn_drop_word(dtile, r), key & 3, da.thr);
            dpv = keep ? dpv * da.inv_keep : 0.f;
          }
          s[mt][r] = keep ? p : 0.f;
          ds[mt][r] = p * (dpv - Dd[qi]);
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {                           // dVᵀ += dOᵀ·P, dKᵀ += Qᵀ·dS
        attn_pv_half<D>(dv, pack2<hb>(s[2 * k2], s[2 * k2 + 1]), Dt + 32 * k2, LDT, col, hgrp);
        attn_pv_half<D>(dk, pack2<hb>(ds[2 * k2], ds[2 * k2 + 1]), Qt + 32 * k2, LDT, col, hgrp);
      }
    }
  }
  if (key < Tk) {
    hb* dst = dk_out + (long long)b * dk_bs + (long long)key * dk_ld + j * D;
    attn_store_tile<D>(dst, dk, scale, hgrp);
    if constexpr (DROP) {   // its own fp32 multiply: as the store's factor it fuses with the fp16 conversion
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) dv[dt] *= da.inv_keep;
    }
    attn_store_tile<D>(dst + v_off, dv, 1.f, hgrp);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// Calls f(std::integral_constant<int, D>, AttnElem<hb>) for the kernel instance of (dt, D): dt 1 = bf16, 2 = fp16,
// D in {64, 128}. -1 when there is none.
template <typename hb> struct AttnElem { using type = hb; };
template <typename F> static int attn_dispatch(int dt, int D, F&& f) {
  if ((dt != 1 && dt != 2) || (D != 64 && D != 128)) return -1;
  if (D == 64) return dt == 1 ? f(std::integral_constant<int, 64>{}, AttnElem<__bf16>{})
                              : f(std::integral_constant<int, 64>{}, AttnElem<_Float16>{});
  return dt == 1 ? f(std::integral_constant<int, 128>{}, AttnElem<__bf16>{})
                 : f(std::integral_constant<int, 128>{}, AttnElem<_Float16>{});
}
// every pointer is 16-byte aligned (null counts as aligned)
static inline bool attn_aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) == 0;
}
