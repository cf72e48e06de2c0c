// Cross attention (flash-style) for gfx950: queries of one sequence (length Tq) attend over the keys / values of
// another (length Tk, its own key-padding mask). bf16 or fp16 in / fp32 accumulate, head dim D in {64, 128}.
// Used by CrossAttentionLayer and TransformerDecoderLayer (encoder-decoder transformers).
//
// Layout (the projections write it directly, a cached memory projection is passed as is):
//   q, out, dout, dq [B, Tq, E]   contiguous, head h at column h*D (E = H*D)
//   kv [B, TkCap, 2E]             K of head h at column h*D, V at E + h*D (the decode cache layout); rows [0, Tk) are
//                                 valid, rows at or beyond Tk are never loaded; the batch stride is TkCap*2E
//   dkv [B, Tk, 2E]               fully written
//   kmask [B, Tk] fp32 (1 = keep) or null;  lse, dq_dot [B, H, Tq] fp32
// There is no causal flag and no dropout instance.
//
// The wave mapping and numerics are those of csrc/attention.hip (transposed scores Sᵀ = K·Qᵀ on
// v_mfma_f32_16x16x32, exp2-domain online softmax, Pᵀ kept in registers as the B operand, fp32 accumulation); what
// differs is that the two axes have their own lengths:
//  * forward / dQ: grid (ceil(Tq/64), B*H), a wave owns 16 queries and loops over the key blocks of Tk;
//  * dK/dV: grid (ceil(Tk/64), B*H), a wave owns 16 keys and loops over the query blocks of Tq;
//  * query rows are bounded by Tq and key rows by Tk, never one by the other.
// No atomics: results are bitwise reproducible. A batch row whose keys are all masked gives zero output, the 1e30
// lse sentinel (so every backward probability is exp2(s - 1e30) = 0) and zero dQ / dK / dV.
#include "attention_mma.h"

// ------------------------------------------------------------------------------------------------ forward
// NB key blocks are staged per round as in attn_fwd_kernel (NB = 2 for D = 64); every thread issues all of the
// round's K and V loads before any LDS store.
template <int D, typename hb, int NB>
__global__ void __launch_bounds__(256) attn_cross_fwd_kernel(const hb* __restrict__ qp, const hb* __restrict__ kv,
                                                             const float* __restrict__ kmask, hb* __restrict__ out,
                                                             float* __restrict__ lse, int Tq, int Tk, int TkCap,
                                                             int H, float scale2) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDK = D + 8, LDV = NB * BLK + 8;
  constexpr int CPR = D / 8, PER = BLK * CPR / 256;              // 16-byte chunks per row / per thread per block
  __shared__ __attribute__((aligned(16))) hb Ks[NB * BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Vt[D * LDV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int E = H * D;
  const long long ld2 = 2LL * E;
  const hb* kbase = kv + (long long)b * TkCap * ld2 + h * D;
  const int q = blockIdx.x * BLK + wave * 16 + col;
  const int qc = min(q, Tq - 1);
  V8<hb> qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = ld8(qp + ((long long)b * Tq + qc) * E + h * D + ks * 32 + 8 * hgrp);
  f4_t acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  float m = kNegInf, l = 0.f;
  const float* mrow = kmask ? kmask + (long long)b * Tk : nullptr;
  const int nkb = (Tk + BLK - 1) / BLK;
  for (int kb0 = 0; kb0 < nkb; kb0 += NB) {
    __syncthreads();
    V8<hb> kr[NB][PER], vr[NB][PER];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int it = 0; it < PER; ++it) {
        const int i = threadIdx.x + it * 256, r = i / CPR, c = i - r * CPR;
        const int row = (kb0 + j) * BLK + r;
        const bool ok = kb0 + j < nkb && row < Tk;
        const hb* src = kbase + (long long)(ok ? row : 0) * ld2 + c * 8;
        kr[j][it] = ok ? ld8(src) : V8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
        vr[j][it] = ok ? ld8(src + E) : V8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int it = 0; it < PER; ++it) {
        const int i = threadIdx.x + it * 256, r = i / CPR, c = i - r * CPR;
        *reinterpret_cast<V8<hb>*>(Ks + (j * BLK + r) * LDK + c * 8) = kr[j][it];
#pragma unroll
        for (int k = 0; k < 8; ++k) Vt[(c * 8 + k) * LDV + j * BLK + r] = vr[j][it][k];
      }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int kb = kb0 + j;
      if (kb >= nkb) break;
      const hb* Kj = Ks + j * BLK * LDK;
      f4_t s[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        s[mt] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s[mt] = mma(ld8(Kj + (mt * 16 + col) * LDK + ks * 32 + 8 * hgrp), qf[ks], s[mt]);
      }
      float bm = kNegInf;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb * BLK + mt * 16 + hgrp * 4 + r;
          bool ok = key < Tk;
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
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const V8<hb> pb = pack2<hb>(s[2 * k2], s[2 * k2 + 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          acc[dt] = mma(ld4x2(Vt + (dt * 16 + col) * LDV + j * BLK + 32 * k2, hgrp), pb, acc[dt]);
      }
    }
  }
  if (q < Tq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    hb* orow = out + ((long long)b * Tq + q) * E + h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const V4<hb> v{tobf<hb>(acc[dt][0] * inv), tobf<hb>(acc[dt][1] * inv), tobf<hb>(acc[dt][2] * inv), tobf<hb>(acc[dt][3] * inv)};
      *reinterpret_cast<V4<hb>*>(orow + dt * 16 + hgrp * 4) = v;
    }
    if (hgrp == 0) lse[(long long)bh * Tq + q] = l > 0.f ? m + log2f(l) : 1e30f;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// Dq[b,h,q] = sum_d dO[q,d] * O[q,d]
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_cross_bwd_pre_kernel(const hb* __restrict__ o, const hb* __restrict__ dout,
                                                                 float* __restrict__ dq_dot, int B, int Tq, int H) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over B*H*Tq
  if (i >= (long long)B * H * Tq) return;
  const int q = (int)(i % Tq);
  const long long bh = i / Tq;
  const int h = (int)(bh % H), b = (int)(bh / H);
  const long long off = ((long long)b * Tq + q) * H * D + h * D;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    const V8<hb> a = ld8(o + off + c * 8), g = ld8(dout + off + c * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (float)a[k] * (float)g[k];
  }
  dq_dot[i] = s;
}

// dQ per query block (forward orientation: query on the lane)
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_cross_bwd_dq_kernel(const hb* __restrict__ qp, const hb* __restrict__ kv,
                                                                const hb* __restrict__ dout,
                                                                const float* __restrict__ kmask,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ dq_dot, hb* __restrict__ dq,
                                                                int Tq, int Tk, int TkCap, int H, float scale2,
                                                                float scale) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDK = D + 8, LDT = BLK + 8;
  __shared__ __attribute__((aligned(16))) hb Ks[BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Vs[BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Kt[D * LDT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int E = H * D;
  const long long ld2 = 2LL * E;
  const hb* kbase = kv + (long long)b * TkCap * ld2 + h * D;
  const int q = blockIdx.x * BLK + wave * 16 + col;
  const int qc = min(q, Tq - 1);
  V8<hb> qf[KS], df[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = ld8(qp + ((long long)b * Tq + qc) * E + h * D + ks * 32 + 8 * hgrp);
    df[ks] = ld8(dout + ((long long)b * Tq + qc) * E + h * D + ks * 32 + 8 * hgrp);
  }
  const float l2 = lse[(long long)bh * Tq + qc];
  const float dd = dq_dot[(long long)bh * Tq + qc];
  f4_t acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  const float* mrow = kmask ? kmask + (long long)b * Tk : nullptr;
  const int nkb = (Tk + BLK - 1) / BLK;
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    stage_rows<D>(Ks, LDK, kbase, ld2, kb * BLK, Tk);
    stage_rows<D>(Vs, LDK, kbase + E, ld2, kb * BLK, Tk);
    stage_rows_t<D>(Kt, LDT, kbase, ld2, kb * BLK, Tk);
    __syncthreads();
    f4_t s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = f4_t{0.f, 0.f, 0.f, 0.f};
      dp[mt] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s[mt] = mma(ld8(Ks + (mt * 16 + col) * LDK + ks * 32 + 8 * hgrp), qf[ks], s[mt]);
        dp[mt] = mma(ld8(Vs + (mt * 16 + col) * LDK + ks * 32 + 8 * hgrp), df[ks], dp[mt]);
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb * BLK + mt * 16 + hgrp * 4 + r;
        bool ok = key < Tk && q < Tq;
        if (ok && mrow) ok = mrow[key] != 0.f;
        const float p = ok ? exp2f(s[mt][r] * scale2 - l2) : 0.f;
        s[mt][r] = p * (dp[mt][r] - dd);                         // dS (w.r.t. the scaled scores)
      }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const V8<hb> sb = pack2<hb>(s[2 * k2], s[2 * k2 + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld4x2(Kt + (dt * 16 + col) * LDT + 32 * k2, hgrp), sb, acc[dt]);
    }
  }
  if (q < Tq) {
    hb* dst = dq + ((long long)b * Tq + q) * E + h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const V4<hb> v{tobf<hb>(acc[dt][0] * scale), tobf<hb>(acc[dt][1] * scale), tobf<hb>(acc[dt][2] * scale),
                       tobf<hb>(acc[dt][3] * scale)};
      *reinterpret_cast<V4<hb>*>(dst + dt * 16 + hgrp * 4) = v;
    }
  }
}

// dK, dV per key block (key on the lane), looping over the query blocks of Tq
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_cross_bwd_dkdv_kernel(const hb* __restrict__ qp, const hb* __restrict__ kv,
                                                                  const hb* __restrict__ dout,
                                                                  const float* __restrict__ kmask,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ dq_dot,
                                                                  hb* __restrict__ dkv, int Tq, int Tk, int TkCap,
                                                                  int H, float scale2, float scale) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDQ = D + 8, LDT = BLK + 8;
  __shared__ __attribute__((aligned(16))) hb Qs[BLK * LDQ];
  __shared__ __attribute__((aligned(16))) hb Ds[BLK * LDQ];
  __shared__ __attribute__((aligned(16))) hb Qt[D * LDT];
  __shared__ __attribute__((aligned(16))) hb Dt[D * LDT];
  __shared__ float Ls[BLK], Dd[BLK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int E = H * D;
  const long long ld2 = 2LL * E;
  const hb* kbase = kv + (long long)b * TkCap * ld2 + h * D;
  const hb* qbase = qp + (long long)b * Tq * E + h * D;
  const hb* dbase = dout + (long long)b * Tq * E + h * D;
  const int key = blockIdx.x * BLK + wave * 16 + col;
  const int kc = min(key, Tk - 1);
  bool kvalid = key < Tk;
  if (kvalid && kmask) kvalid = kmask[(long long)b * Tk + key] != 0.f;
  V8<hb> kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = ld8(kbase + (long long)kc * ld2 + ks * 32 + 8 * hgrp);
    vf[ks] = ld8(kbase + (long long)kc * ld2 + E + ks * 32 + 8 * hgrp);
  }
  f4_t dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  const int nqb = (Tq + BLK - 1) / BLK;
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();
    stage_rows<D>(Qs, LDQ, qbase, E, qb * BLK, Tq);
    stage_rows<D>(Ds, LDQ, dbase, E, qb * BLK, Tq);
    stage_rows_t<D>(Qt, LDT, qbase, E, qb * BLK, Tq);
    stage_rows_t<D>(Dt, LDT, dbase, E, qb * BLK, Tq);
    if (threadIdx.x < BLK) {
      const int qq = min(qb * BLK + (int)threadIdx.x, Tq - 1);
      Ls[threadIdx.x] = lse[(long long)bh * Tq + qq];
      Dd[threadIdx.x] = dq_dot[(long long)bh * Tq + qq];
    }
    __syncthreads();
    f4_t s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = f4_t{0.f, 0.f, 0.f, 0.f};
      dp[mt] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s[mt] = mma(ld8(Qs + (mt * 16 + col) * LDQ + ks * 32 + 8 * hgrp), kf[ks], s[mt]);
        dp[mt] = mma(ld8(Ds + (mt * 16 + col) * LDQ + ks * 32 + 8 * hgrp), vf[ks], dp[mt]);
      }
    }
    f4_t ds[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = mt * 16 + hgrp * 4 + r, q = qb * BLK + qi;
        const bool ok = kvalid && q < Tq;
        const float p = ok ? exp2f(s[mt][r] * scale2 - Ls[qi]) : 0.f;
        s[mt][r] = p;
        ds[mt][r] = p * (dp[mt][r] - Dd[qi]);
      }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const V8<hb> pb = pack2<hb>(s[2 * k2], s[2 * k2 + 1]);
      const V8<hb> sb = pack2<hb>(ds[2 * k2], ds[2 * k2 + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dv[dt] = mma(ld4x2(Dt + (dt * 16 + col) * LDT + 32 * k2, hgrp), pb, dv[dt]);
        dk[dt] = mma(ld4x2(Qt + (dt * 16 + col) * LDT + 32 * k2, hgrp), sb, dk[dt]);
      }
    }
  }
  if (key < Tk) {
    hb* dst = dkv + ((long long)b * Tk + key) * ld2 + h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const V4<hb> kk{tobf<hb>(dk[dt][0] * scale), tobf<hb>(dk[dt][1] * scale), tobf<hb>(dk[dt][2] * scale),
                        tobf<hb>(dk[dt][3] * scale)};
      const V4<hb> vv{tobf<hb>(dv[dt][0]), tobf<hb>(dv[dt][1]), tobf<hb>(dv[dt][2]), tobf<hb>(dv[dt][3])};
      *reinterpret_cast<V4<hb>*>(dst + dt * 16 + hgrp * 4) = kk;
      *reinterpret_cast<V4<hb>*>(dst + E + dt * 16 + hgrp * 4) = vv;
    }
  }
}

// ------------------------------------------------------------------------------------------------ launch
template <int D, typename hb>
static int cross_fwd_l(const void* q, const void* kv, const float* kmask, void* out, float* lse, int B, int Tq, int Tk,
                       int TkCap, int H, float scale, hipStream_t s) {
  const dim3 grid((Tq + BLK - 1) / BLK, B * H);
  constexpr int NB = D == 64 ? 2 : 1;
  hipLaunchKernelGGL((attn_cross_fwd_kernel<D, hb, NB>), grid, dim3(256), 0, s, (const hb*)q, (const hb*)kv, kmask,
                     (hb*)out, lse, Tq, Tk, TkCap, H, scale * kLog2e);
  return (int)hipGetLastError();
}

template <int D, typename hb>
static int cross_bwd_l(const void* q, const void* kv, const void* out, const void* dout, const float* kmask,
                       const float* lse, float* dq_dot, void* dq, void* dkv, int B, int Tq, int Tk, int TkCap, int H,
                       float scale, hipStream_t s) {
  const long long n = (long long)B * H * Tq;
  hipLaunchKernelGGL((attn_cross_bwd_pre_kernel<D, hb>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     (const hb*)out, (const hb*)dout, dq_dot, B, Tq, H);
  hipLaunchKernelGGL((attn_cross_bwd_dkdv_kernel<D, hb>), dim3((Tk + BLK - 1) / BLK, B * H), dim3(256), 0, s,
                     (const hb*)q, (const hb*)kv, (const hb*)dout, kmask, lse, dq_dot, (hb*)dkv, Tq, Tk, TkCap, H,
                     scale * kLog2e, scale);
  hipLaunchKernelGGL((attn_cross_bwd_dq_kernel<D, hb>), dim3((Tq + BLK - 1) / BLK, B * H), dim3(256), 0, s,
                     (const hb*)q, (const hb*)kv, (const hb*)dout, kmask, lse, dq_dot, (hb*)dq, Tq, Tk, TkCap, H,
                     scale * kLog2e, scale);
  return (int)hipGetLastError();
}

static bool cross_al16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

static bool cross_shape_ok(int dt, int B, int Tq, int Tk, int TkCap, int H, int D) {
  if (B < 1 || Tq < 1 || Tk < 1 || H < 1 || (dt != 1 && dt != 2)) return false;
  if (D != 64 && D != 128) return false;
  return Tk <= TkCap && (long long)B * H <= 65535;
}

// dt: 1 = bf16, 2 = fp16. q [B,Tq,H*D]; kv [B,TkCap,2*H*D] with rows [0,Tk) valid; kmask [B,Tk] fp32 or null;
// out [B,Tq,H*D]; lse [B,H,Tq] fp32. -1 (nothing written) = unsupported dtype / head size, Tk > TkCap,
// B*H > 65535 or an operand that is not 16-byte aligned.
DL4J_API int dl4j_attn_cross_fwd_dt(int dt, const void* q, const void* kv, const float* kmask, void* out, float* lse,
                                    int B, int Tq, int Tk, int TkCap, int H, int D, float scale, hipStream_t s) {
  if (!cross_shape_ok(dt, B, Tq, Tk, TkCap, H, D)) return -1;
  if (!q || !kv || !out || !lse || !cross_al16(q) || !cross_al16(kv) || !cross_al16(out)) return -1;
#define CROSS_FWD(DD, HB) cross_fwd_l<DD, HB>(q, kv, kmask, out, lse, B, Tq, Tk, TkCap, H, scale, s)
  if (D == 64) return dt == 1 ? CROSS_FWD(64, __bf16) : CROSS_FWD(64, _Float16);
  return dt == 1 ? CROSS_FWD(128, __bf16) : CROSS_FWD(128, _Float16);
#undef CROSS_FWD
}

// dout [B,Tq,H*D]; dq_dot: fp32 workspace [B,H,Tq]; dq [B,Tq,H*D] and dkv [B,Tk,2*H*D] (both fully written).
DL4J_API int dl4j_attn_cross_bwd_dt(int dt, const void* q, const void* kv, const void* out, const void* dout,
                                    const float* kmask, const float* lse, float* dq_dot, void* dq, void* dkv, int B,
                                    int Tq, int Tk, int TkCap, int H, int D, float scale, hipStream_t s) {
  if (!cross_shape_ok(dt, B, Tq, Tk, TkCap, H, D)) return -1;
  if (!q || !kv || !out || !dout || !lse || !dq_dot || !dq || !dkv) return -1;
  if (!cross_al16(q) || !cross_al16(kv) || !cross_al16(out) || !cross_al16(dout) || !cross_al16(dq) ||
      !cross_al16(dkv))
    return -1;
#define CROSS_BWD(DD, HB) \
  cross_bwd_l<DD, HB>(q, kv, out, dout, kmask, lse, dq_dot, dq, dkv, B, Tq, Tk, TkCap, H, scale, s)
  if (D == 64) return dt == 1 ? CROSS_BWD(64, __bf16) : CROSS_BWD(64, _Float16);
  return dt == 1 ? CROSS_BWD(128, __bf16) : CROSS_BWD(128, _Float16);
#undef CROSS_BWD
}
