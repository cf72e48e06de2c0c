// Cached incremental decoding for the causal transformer layers (rnnTimeStep): a key/value cache per layer and an
// attention kernel from a few new queries to the stored history, for gfx950, bf16 or fp16 in / fp32 accumulate,
// head dim D in {64, 128}.
//
// Cache layout: kv[B, Tcap, 2*E] (E = H*D) in the compute dtype; K of head h at column h*D, V at E + h*D — the fused
// projection layout of csrc/attention.hip minus the Q block. Tcap is a multiple of 64; rows at or beyond the valid
// length hold whatever was left there and are never used.
//
//  * attn_kv_append_kernel copies the K and V column blocks of qkv[B, Tn, 3E] to rows [pos, pos + Tn) of the cache
//    (16-byte vectors).
//  * attn_decode_kernel: queries are the Q columns of qkv[B, Tn, 3E], keys / values rows [0, pos + Tn) of the cache
//    (the new rows already appended); query i sees keys <= pos + i. The wave mapping and the per-block arithmetic
//    are the forward ones of csrc/attention_body.h, written out here: built from that header's inner-step helpers the
//    kernel computes the same bits but measures 1-2 % slower at a 128-key history (profiles/attention_unify.txt).
//    The block stages each 64-key block cooperatively (K row-major, V transposed), with the next block's global loads
//    in flight during the current block's MFMAs. Waves whose 16 queries all lie beyond Tn only stage (at Tn <= 16 that is three
//    of four; the kernel is bound by the cache read).
//  * The keys are split: grid (splits, B*H, ceil(Tn/64)); split s covers the contiguous 64-key blocks
//    [s*nkb/S, (s+1)*nkb/S). One split normalises and writes out directly; several write fp32 partials (running max
//    m in the exp2 domain, sum l, unnormalised accumulator) to a workspace and attn_decode_combine_kernel merges
//    them in the fixed order s = 0 .. S-1 — no atomics, bitwise reproducible for a given split count. A split that
//    is causally empty for a query leaves (-inf, 0, 0) and is skipped by the merge.
//  * Ragged batches (prompts of different lengths, right-padded): the host keeps one upper bound pos and a device
//    array shortfall[b] = what row b lacks against it, written once per sequence. The *_ragged_kernel variants run
//    the same bodies at pos - shortfall[b]; for a row with at least S key blocks the result is the bits the uniform
//    kernel gives that row alone at its own position with the same S.
//  * FP8 cache (opt-in): kv8[B, Tcap, R] bytes, R = 2E + roundup16(2H). A group is the D values of one token, one
//    head, K or V: amax = max |x|, ex the smallest integer with amax * 2^-ex <= 448 (0 for an all-zero group, clamped
//    into [-126, 127]), code = e4m3fn(x * 2^-ex) (OCP, round to nearest even; the scaling is exact and nothing
//    saturates), value = code * 2^ex. K codes of head h at byte h*D, V codes at E + h*D, K's scale byte ex + 127 at
//    2E + h, V's at 2E + H + h, zero pad up to R. attn_kv_append_fp8_kernel quantises and writes; the decode body
//    takes the cache side as a policy (KvCache16 / KvCacheFp8): the fp8 one loads 16 codes per 16-byte vector plus
//    the row's two scale bytes and converts while staging (v_cvt_scalef32_pk_{bf16,f16}_fp8), writing the same Ks / Vt
//    images — from the first barrier on the two are one code, so the fp8 kernel gives the bits of the 16-bit kernel
//    on the dequantised cache.
//
// Grouped-query attention (the *_gqa_dt entry points): H query heads share Hkv key/value heads, G = H / Hkv an
// integer, Ekv = Hkv*D; query head h uses kv head h / G. Layouts:
//   qkv [B, Tn, E + 2*Ekv]        Q of head h at column h*D, K of kv head j at E + j*D, V at E + Ekv + j*D
//   kv [B, Tcap, 2*Ekv]           K of kv head j at column j*D, V at Ekv + j*D
//   kv8 [B, Tcap, R] bytes        R = 2*Ekv + roundup16(2*Hkv): the fp8 format above with Hkv heads (same groups,
//                                 scales and codes)
//   out [B, Tn, E]
//  * The append kernels take the source row width and the K column offset and copy / quantise 2*Ekv columns.
//  * Decode: grid (splits, B*Hkv, ceil(Tn*G/64)). The 64 lane-columns of a block are SLOTS r = i*G + g, query-major:
//    chunk query i = r / G, group member g = r % G. A lane loads the Q fragment of row i, head j*G + g, cuts at
//    key <= pos + i and writes out[b, i, (j*G + g)*D ..]; the block stages each 64-key block of kv head j once for
//    all of them, so the cache bytes read per step shrink by G and at Tn = 1 the G query heads fill lanes and waves
//    that only staged. A wave is active when any of its 16 slots is below Tn*G; the tile's last visible key block
//    follows from its largest i. Split partials go to the workspace slot of (b*H + h, i, split), so the merge kernel
//    is the one above. Staging, prefetch, online softmax and the cache policies are the one body: G = 1 (GQA = false)
//    is a compile-time constant there and gives the multi-head kernels as they were; for a given split count the GQA
//    result is bitwise what those give on the cache with every kv head repeated G times.
#include "attention_body.h"

// ------------------------------------------------------------------------------------------------ cache policies
// What attn_decode_body needs from a cache: elem (the pointer's element type), CPR 16-byte chunks per D columns of a
// row, each CW elements wide and NV fragments of 8 hb, row_ld(E, H) the row stride in elements, chunk / scale_t as the
// registers of one chunk in flight, load / zero. V sits E elements after K in both. With NV == 1 a chunk is the 8 hb
// as they are staged; with NV > 1 it holds codes: load_scale gives the group's scale and piece(.., j) fragment j in hb.
// The scale registers and the conversion are kept out of the NV == 1 instantiations at compile time (if constexpr):
// with them in, dead as they are there, the compiler schedules those kernels differently.
template <int D, typename hb> struct KvCache16 {
  using elem = hb;
  using chunk = V8<hb>;
  struct scale_t {};
  static constexpr int CPR = D / 8, NV = 1, CW = 8;
  static __device__ __forceinline__ long long row_ld(int E, int) { return 2LL * E; }
  static __device__ __forceinline__ chunk load(const hb* p) { return ld8(p); }
  static __device__ __forceinline__ chunk zero() { return V8<hb>{0, 0, 0, 0, 0, 0, 0, 0}; }
};

__device__ __forceinline__ V8<__bf16> fp8x4x2_to(unsigned a, unsigned b, float sc, __bf16) {
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, false);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, true);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, false);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, true);
  return V8<__bf16>{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
__device__ __forceinline__ V8<_Float16> fp8x4x2_to(unsigned a, unsigned b, float sc, _Float16) {
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(a, sc, false);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(a, sc, true);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(b, sc, false);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(b, sc, true);
  return V8<_Float16>{(_Float16)p0[0], (_Float16)p0[1], (_Float16)p1[0], (_Float16)p1[1],
                      (_Float16)p2[0], (_Float16)p2[1], (_Float16)p3[0], (_Float16)p3[1]};
}

// rows of R(E, H) bytes; the head's K codes at the row pointer, V codes E bytes on, the scale bytes at 2E - h*D
template <int D, typename hb> struct KvCacheFp8 {
  using elem = unsigned char;
  using chunk = uint4;                                           // 16 codes
  using scale_t = float;                                         // 2^ex
  static constexpr int CPR = D / 16, NV = 2, CW = 16;
  static __device__ __forceinline__ long long row_ld(int E, int H) { return 2LL * E + ((2 * H + 15) & ~15); }
  static __device__ __forceinline__ chunk load(const elem* p) { return *reinterpret_cast<const uint4*>(p); }
  static __device__ __forceinline__ chunk zero() { return make_uint4(0u, 0u, 0u, 0u); }
  // row points at the head's K codes (byte h*D of the cache row)
  static __device__ __forceinline__ scale_t load_scale(const elem* row, int E, int H, int h, bool v) {
    return __uint_as_float((unsigned)row[2 * E - h * D + (v ? H : 0) + h] << 23);
  }
  static __device__ __forceinline__ V8<hb> piece(const chunk& v, scale_t sc, int j) {
    return j == 0 ? fp8x4x2_to(v.x, v.y, sc, hb{}) : fp8x4x2_to(v.z, v.w, sc, hb{});
  }
};

// partial workspace for S splits: acc[((bh*Tn + q)*S + s)*D + d] (16-byte aligned rows), then ml[(bh*Tn + q)*S + s][2]
// holding (m, l)
// The body takes the position of its own batch row: the uniform kernel passes the host's pos, the ragged one
// pos - shortfall[b] (everything below — key-block count, split ranges, causal cut, zero staging — follows from it).
// GQA: the cache side (row stride, V offset, scale bytes) is that of Hkv heads, the lane-columns are slots.
// WIN: query i sees keys pos + i - window < k <= pos + i; the key blocks are [kb_first, nkb) with kb_first the first
// block the tile's smallest query sees, the S splits divide that range and the blocks before it are never read.
template <int D, typename hb, typename CP = KvCache16<D, hb>, bool GQA = false, bool WIN = false>
__device__ __forceinline__ void attn_decode_body(const hb* __restrict__ qkv, const typename CP::elem* __restrict__ kv,
                                                 hb* __restrict__ out, float* __restrict__ ws, int Tn, int H, int pos,
                                                 int Tcap, int S, float scale2, int Garg = 1, int window = 0) {
  constexpr int KS = D / 32, DT = D / 16;
  constexpr int LDK = D + 8, LDV = BLK + 8;
  constexpr int CPR = CP::CPR, PER = BLK * CPR / 256;            // 16-byte chunks per row / per thread per block
  constexpr int NV = CP::NV;                                     // fragments of 8 hb in a chunk
  __shared__ __attribute__((aligned(16))) hb Ks[BLK * LDK];
  __shared__ __attribute__((aligned(16))) hb Vt[D * LDV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, hgrp = lane >> 4;
  const int G = GQA ? Garg : 1, Hkv = GQA ? H / G : H;           // the cache holds Hkv heads
  const int split = blockIdx.x, bj = blockIdx.y, b = bj / Hkv, j = bj - b * Hkv;
  const int E = H * D, Ekv = GQA ? Hkv * D : E, L = pos + Tn;
  const long long ld3 = GQA ? (long long)E + 2LL * Ekv : 3LL * E, ld2 = CP::row_ld(Ekv, Hkv);
  const typename CP::elem* kbase = kv + (long long)b * Tcap * ld2 + j * D;
  const int q0 = blockIdx.z * BLK;
  const int slot = q0 + wave * 16 + col;                         // r = i*G + g
  const int nslots = GQA ? Tn * G : Tn;
  const int qi = GQA ? slot / G : slot;                          // index in the chunk; its position is pos + qi
  const int h = GQA ? j * G + (slot - qi * G) : j;               // the lane's query head
  const int bh = GQA ? b * H + h : bj;
  const bool active = q0 + wave * 16 < nslots;                   // wave-uniform: any slot of this wave's 16 exists
  const int qc = min(qi, Tn - 1);
  const hb* qbase = qkv + (long long)b * Tn * ld3 + h * D;
  V8<hb> qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = ld8(qbase + (long long)qc * ld3 + ks * 32 + 8 * hgrp);
  f4_t acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = f4_t{0.f, 0.f, 0.f, 0.f};
  float m = kNegInf, l = 0.f;
  // this split's key blocks, cut at the last block any query of the tile can see
  const int nkb = (L + BLK - 1) / BLK;
  int kb_first = 0;                                              // WIN: the first block the tile's smallest query sees
  if constexpr (WIN) kb_first = max(0, pos + (GQA ? q0 / G : q0) - window + 1) / BLK;
  const int nwb = nkb - kb_first;
  const int kb_lo = kb_first + (int)((long long)split * nwb / S);
  const int i_hi = GQA ? (min(q0 + BLK, nslots) - 1) / G : min(q0 + BLK, Tn) - 1;   // the tile's largest query
  const int kb_hi = min(kb_first + (int)((long long)(split + 1) * nwb / S), (pos + i_hi) / BLK + 1);
  typename CP::chunk kr[PER], vr[PER];
  typename CP::scale_t ksc[PER], vsc[PER];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      const int i = threadIdx.x + it * 256, r = i / CPR, c = i - r * CPR;
      const int row = kb * BLK + r;
      const bool ok = row < L;                                   // rows past the valid length are staged as zeros
      const typename CP::elem* src = kbase + (long long)(ok ? row : 0) * ld2 + c * CP::CW;
      kr[it] = ok ? CP::load(src) : CP::zero();
      vr[it] = ok ? CP::load(src + Ekv) : CP::zero();
      if constexpr (NV > 1) {
        ksc[it] = ok ? CP::load_scale(src - c * CP::CW, Ekv, Hkv, j, false) : typename CP::scale_t{};
        vsc[it] = ok ? CP::load_scale(src - c * CP::CW, Ekv, Hkv, j, true) : typename CP::scale_t{};
      }
    }
  };
  if (kb_lo < kb_hi) fetch(kb_lo);
  for (int kb = kb_lo; kb < kb_hi; ++kb) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      const int i = threadIdx.x + it * 256, r = i / CPR, c = i - r * CPR;
      if constexpr (NV == 1) {
        *reinterpret_cast<V8<hb>*>(Ks + r * LDK + c * 8) = kr[it];
#pragma unroll
        for (int k = 0; k < 8; ++k) Vt[(c * 8 + k) * LDV + r] = vr[it][k];
      } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int cj = c * NV + j;                             // the 8-column fragment
          *reinterpret_cast<V8<hb>*>(Ks + r * LDK + cj * 8) = CP::piece(kr[it], ksc[it], j);
          const V8<hb> vj = CP::piece(vr[it], vsc[it], j);
#pragma unroll
          for (int k = 0; k < 8; ++k) Vt[(cj * 8 + k) * LDV + r] = vj[k];
        }
      }
    }
    __syncthreads();
    if (kb + 1 < kb_hi) fetch(kb + 1);
    if (!active) continue;
    f4_t s[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s[mt] = mma(ld8(Ks + (mt * 16 + col) * LDK + ks * 32 + 8 * hgrp), qf[ks], s[mt]);
    }
    float bm = kNegInf;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb * BLK + mt * 16 + hgrp * 4 + r;
        float v;
        if constexpr (WIN)
          v = (key < L && key <= pos + qi && key > pos + qi - window) ? s[mt][r] * scale2 : kNegInf;
        else
          v = (key < L && key <= pos + qi) ? s[mt][r] * scale2 : kNegInf;
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
      for (int dt = 0; dt < DT; ++dt) acc[dt] = mma(ld4x2(Vt + (dt * 16 + col) * LDV + 32 * k2, hgrp), pb, acc[dt]);
    }
  }
  if (qi >= Tn) return;
  if (S == 1) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    hb* orow = out + ((long long)b * Tn + qi) * E + h * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const V4<hb> v{tobf<hb>(acc[dt][0] * inv), tobf<hb>(acc[dt][1] * inv), tobf<hb>(acc[dt][2] * inv), tobf<hb>(acc[dt][3] * inv)};
      *reinterpret_cast<V4<hb>*>(orow + dt * 16 + hgrp * 4) = v;
    }
    return;
  }
  const long long wslot = ((long long)bh * Tn + qi) * S + split;
  const long long nslot = (long long)gridDim.y * G * Tn * S;     // B*H*Tn*S
  if (hgrp == 0) {
    ws[nslot * D + wslot * 2] = m;
    ws[nslot * D + wslot * 2 + 1] = l;
  }
  float* arow = ws + wslot * D;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f4_t*>(arow + dt * 16 + hgrp * 4) = acc[dt];
}

template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_decode_kernel(const hb* __restrict__ qkv, const hb* __restrict__ kv,
                                                          hb* __restrict__ out, float* __restrict__ ws, int Tn, int H,
                                                          int pos, int Tcap, int S, float scale2) {
  attn_decode_body<D, hb>(qkv, kv, out, ws, Tn, H, pos, Tcap, S, scale2);
}

// Per-row positions: pos is the host's upper bound (it sizes the grid and the split count S), shortfall[b] what row
// b lacks against it, clamped into [0, pos]. A row with fewer key blocks than S leaves its upper splits empty:
// they write the (-inf, 0, 0) partial the merge skips.
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_decode_ragged_kernel(const hb* __restrict__ qkv, const hb* __restrict__ kv,
                                                                 hb* __restrict__ out, float* __restrict__ ws, int Tn,
                                                                 int H, int pos, int Tcap, int S, float scale2,
                                                                 const int* __restrict__ shortfall) {
  const int b = blockIdx.y / H;
  attn_decode_body<D, hb>(qkv, kv, out, ws, Tn, H, pos - min(max(shortfall[b], 0), pos), Tcap, S, scale2);
}

// The same two kernels over the fp8 cache kv8[B, Tcap, R].
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_decode_fp8_kernel(const hb* __restrict__ qkv,
                                                              const unsigned char* __restrict__ kv8,
                                                              hb* __restrict__ out, float* __restrict__ ws, int Tn,
                                                              int H, int pos, int Tcap, int S, float scale2) {
  attn_decode_body<D, hb, KvCacheFp8<D, hb>>(qkv, kv8, out, ws, Tn, H, pos, Tcap, S, scale2);
}
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_decode_fp8_ragged_kernel(const hb* __restrict__ qkv,
                                                                     const unsigned char* __restrict__ kv8,
                                                                     hb* __restrict__ out, float* __restrict__ ws,
                                                                     int Tn, int H, int pos, int Tcap, int S,
                                                                     float scale2, const int* __restrict__ shortfall) {
  const int b = blockIdx.y / H;
  attn_decode_body<D, hb, KvCacheFp8<D, hb>>(qkv, kv8, out, ws, Tn, H, pos - min(max(shortfall[b], 0), pos), Tcap, S,
                                             scale2);
}

// Grouped heads, all four variants (CP: 16-bit or fp8 cache; shortfall null = every row at pos): grid.y = B*Hkv,
// grid.z tiles the Tn*G slots.
template <int D, typename hb, typename CP>
__global__ void __launch_bounds__(256) attn_decode_gqa_kernel(const hb* __restrict__ qkv,
                                                              const typename CP::elem* __restrict__ kv,
                                                              hb* __restrict__ out, float* __restrict__ ws, int Tn,
                                                              int H, int Hkv, int pos, int Tcap, int S, float scale2,
                                                              const int* __restrict__ shortfall) {
  const int b = blockIdx.y / Hkv;
  const int pb = shortfall ? pos - min(max(shortfall[b], 0), pos) : pos;
  attn_decode_body<D, hb, CP, true>(qkv, kv, out, ws, Tn, H, pb, Tcap, S, scale2, H / Hkv);
}

// The sliding-window variants, all eight from one kernel (CP: 16-bit or fp8 cache; GQA = false is Hkv == H with the
// compile-time group size; shortfall null = every row at pos): the body with WIN = true at the row's own position.
template <int D, typename hb, typename CP, bool GQA>
__global__ void __launch_bounds__(256) attn_decode_win_kernel(const hb* __restrict__ qkv,
                                                              const typename CP::elem* __restrict__ kv,
                                                              hb* __restrict__ out, float* __restrict__ ws, int Tn,
                                                              int H, int Hkv, int pos, int Tcap, int S, float scale2,
                                                              int window, const int* __restrict__ shortfall) {
  const int b = blockIdx.y / Hkv;
  const int pb = shortfall ? pos - min(max(shortfall[b], 0), pos) : pos;
  attn_decode_body<D, hb, CP, GQA, true>(qkv, kv, out, ws, Tn, H, pb, Tcap, S, scale2, H / Hkv, window);
}

// out[b, q, h*D + d] = sum_s acc_s[d] 2^(m_s - M) / sum_s l_s 2^(m_s - M), M = max_s m_s, in the order s = 0 .. S-1;
// one thread per (bh, q, 4 consecutive d)
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_decode_combine_kernel(const float* __restrict__ ws, hb* __restrict__ out,
                                                                  long long BH, int Tn, int H, int S) {
  constexpr int DQ = D / 4;
  const long long nrow = BH * Tn;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrow * DQ) return;
  const long long row = i / DQ;                                  // bh*Tn + q
  const int d4 = (int)(i - row * DQ);
  const long long bh = row / Tn;
  const int q = (int)(row - bh * Tn);
  const int h = (int)(bh % H);
  const long long b = bh / H;
  const float* ac = ws + row * S * D + d4 * 4;
  const float* ml = ws + nrow * S * D + row * S * 2;
  // the partials are read CH splits at a time, all loads of a chunk issued before their first use: a thread's merge
  // costs ceil(S / CH) memory round trips, not S. The sums still run in the order s = 0 .. S-1.
  constexpr int CH = 8;
  float M = kNegInf;
  for (int s0 = 0; s0 < S; s0 += CH) {
    float mv[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) mv[j] = ml[2 * min(s0 + j, S - 1)];
#pragma unroll
    for (int j = 0; j < CH; ++j) M = fmaxf(M, mv[j]);
  }
  float l = 0.f;
  f4_t o{0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < S; s0 += CH) {
    float mv[CH], lv[CH];
    f4_t av[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int s = min(s0 + j, S - 1);
      mv[j] = ml[2 * s];
      lv[j] = ml[2 * s + 1];
      av[j] = *reinterpret_cast<const f4_t*>(ac + (long long)s * D);
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      if (s0 + j >= S || mv[j] == kNegInf) continue;             // past the end, or a causally empty split
      const float w = exp2f(mv[j] - M);
      l += lv[j] * w;
      o += av[j] * w;
    }
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  const V4<hb> v{tobf<hb>(o[0] * inv), tobf<hb>(o[1] * inv), tobf<hb>(o[2] * inv), tobf<hb>(o[3] * inv)};
  *reinterpret_cast<V4<hb>*>(out + ((b * Tn + q) * H + h) * D + d4 * 4) = v;
}

// In 16-byte chunks (EC per Ekv columns; the source row is LDC chunks wide with its K columns at chunk KC): chunk c
// of the 2*Ekv K|V columns of qkv row (b, t) -> kv row (b, pos + t)
__global__ void __launch_bounds__(256) attn_kv_append_kernel(const uint4* __restrict__ qkv, uint4* __restrict__ kv,
                                                             long long total, int Tn, int EC, int LDC, int KC, int pos,
                                                             int Tcap) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (2 * EC));
  const long long bt = i / (2 * EC);                             // b*Tn + t
  const int t = (int)(bt % Tn);
  const long long b = bt / Tn;
  kv[(b * Tcap + pos + t) * (2LL * EC) + c] = qkv[bt * (long long)LDC + KC + c];
}

// The same copy to rows [pos - shortfall[b], pos - shortfall[b] + Tn) of batch row b; the shortfall is clamped into
// [0, pos], so whatever the array holds no write leaves rows [0, pos + Tn) of its own batch row.
__global__ void __launch_bounds__(256) attn_kv_append_ragged_kernel(const uint4* __restrict__ qkv,
                                                                    uint4* __restrict__ kv, long long total, int Tn,
                                                                    int EC, int LDC, int KC, int pos, int Tcap,
                                                                    const int* __restrict__ shortfall) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (2 * EC));
  const long long bt = i / (2 * EC);                             // b*Tn + t
  const int t = (int)(bt % Tn);
  const long long b = bt / Tn;
  const int pb = pos - min(max(shortfall[b], 0), pos);
  kv[(b * Tcap + pb + t) * (2LL * EC) + c] = qkv[bt * (long long)LDC + KC + c];
}

// FP8 append: D / 16 lanes per (token, head, K|V) group, 16 values each. The group's amax is reduced across its lanes
// (they sit in one wave: 4 or 8 consecutive lanes), every lane writes its 16 codes as one 16-byte vector and lane 0
// the scale byte; the last group of a token also zeroes the pad bytes. shortfall: null (every row at pos) or the
// per-row array, clamped into [0, pos] as in attn_kv_append_ragged_kernel. H is the number of heads the cache holds
// (Hkv); the source row is ld elements wide with its K columns at koff.
template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_kv_append_fp8_kernel(const hb* __restrict__ qkv,
                                                                 unsigned char* __restrict__ kv8, long long total,
                                                                 int Tn, int H, int ld, int koff, int pos, int Tcap,
                                                                 const int* __restrict__ shortfall) {
  constexpr int LPG = D / 16;                                    // lanes per group
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;                                        // whole groups leave: total is a multiple of LPG
  const int c = (int)(i % LPG);
  const long long gi = i / LPG;
  const int g = (int)(gi % (2 * H));                             // K heads 0 .. H-1, then V heads
  const long long bt = gi / (2 * H);                             // b*Tn + t
  const int t = (int)(bt % Tn);
  const long long b = bt / Tn;
  const int E = H * D, tail = (2 * H + 15) & ~15;
  const hb* src = qkv + bt * (long long)ld + koff + g * D + c * 16;
  const V8<hb> lo = ld8(src), hi = ld8(src + 8);
  float x[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    x[k] = (float)lo[k];
    x[8 + k] = (float)hi[k];
  }
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) amax = fmaxf(amax, fabsf(x[k]));
#pragma unroll
  for (int o = 1; o < LPG; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  // amax = m * 2^e, m in [0.5, 1): 448 = 0.875 * 2^9
  int e;
  const float m = frexpf(amax, &e);
  int ex = amax > 0.f ? (m <= 0.875f ? e - 9 : e - 8) : 0;
  ex = min(max(ex, -126), 127);
  unsigned w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x[4 * k], -ex), ldexpf(x[4 * k + 1], -ex), 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x[4 * k + 2], -ex), ldexpf(x[4 * k + 3], -ex), v, true);
    w[k] = (unsigned)v;
  }
  const int pb = shortfall ? pos - min(max(shortfall[b], 0), pos) : pos;
  unsigned char* row = kv8 + (b * Tcap + pb + t) * (2LL * E + tail);
  *reinterpret_cast<uint4*>(row + g * D + c * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  if (c == 0) {
    row[2 * E + g] = (unsigned char)(ex + 127);
    if (g == 2 * H - 1)
      for (int p = 2 * H; p < tail; ++p) row[2 * E + p] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ launch
// Default split count, from the measurements of tools/bench_decode.py --kernel --sweep (profiles/decode_attention.txt):
// a block's pass over its key blocks is a chain of dependent memory round trips, so short chains on many blocks win
// until a split is down to one key block (then the merge launch costs more than it saves) or the merge itself, whose
// cost grows with the split count, shows: two key blocks per split, at most 16 splits. That held from 12 to 384
// (batch x head) blocks; splitting stops where the unsplit grid alone exceeds the blocks resident at once (4 per
// compute unit at this kernel's registers for D = 64) — a bound by residency, not measured.
static constexpr int kDecodeCUs = 256;            // MI355X compute units
static constexpr int kDecodeResidentPerCU = 4;
static constexpr int kDecodeMinBlocksPerSplit = 2;
static constexpr int kDecodeMaxSplits = 16;

static int decode_nkb(int L) { return (L + BLK - 1) / BLK; }
static int decode_clamp_splits(int splits, int L) { return splits < decode_nkb(L) ? splits : decode_nkb(L); }

static bool decode_shape_ok(int dt, int B, int Tn, int H, int Hkv, int D, int pos, int Tcap) {
  if (B < 1 || Tn < 1 || H < 1 || pos < 0 || Tcap < 1 || (dt != 1 && dt != 2) || (D != 64 && D != 128)) return false;
  if (Hkv < 1 || H % Hkv) return false;
  if (Tcap % BLK || (long long)pos + Tn > Tcap) return false;
  const long long tiles = ((long long)Tn * (H / Hkv) + BLK - 1) / BLK;
  if ((long long)B * Hkv > 65535 || tiles > 65535) return false;               // grid.y / grid.z
  return true;
}

// Default split count for keys [0, L) (see the constants above): min(16, key blocks / 2), one split when the
// (batch x kv head x slot tile) grid fills the device by itself. A pure function of its arguments (no timing), so a
// run is reproducible across processes.
DL4J_API int dl4j_attn_decode_splits_gqa(int B, int Tn, int H, int Hkv, int D, int L) {
  if (B < 1 || Tn < 1 || H < 1 || Hkv < 1 || H % Hkv || L < 1 || (D != 64 && D != 128)) return 1;
  const long long base = (long long)B * Hkv * (((long long)Tn * (H / Hkv) + BLK - 1) / BLK);
  if (base >= (long long)kDecodeCUs * kDecodeResidentPerCU) return 1;
  int s = decode_nkb(L) / kDecodeMinBlocksPerSplit;
  if (s > kDecodeMaxSplits) s = kDecodeMaxSplits;
  return s < 1 ? 1 : s;
}
DL4J_API int dl4j_attn_decode_splits(int B, int Tn, int H, int D, int L) {
  return dl4j_attn_decode_splits_gqa(B, Tn, H, H, D, L);
}

// fp32 workspace of dl4j_attn_decode_dt for a requested split count (enough for any clamped one); 0 for one split.
// The partials are per QUERY head, so the size does not depend on Hkv (0 for an Hkv that does not divide H).
DL4J_API long long dl4j_attn_decode_ws_bytes_gqa(int B, int Tn, int H, int Hkv, int D, int splits) {
  if (B < 1 || Tn < 1 || H < 1 || Hkv < 1 || H % Hkv || D < 1 || splits <= 1) return 0;
  return (long long)B * H * Tn * splits * (D + 2) * (long long)sizeof(float);
}
DL4J_API long long dl4j_attn_decode_ws_bytes(int B, int Tn, int H, int D, int splits) {
  return dl4j_attn_decode_ws_bytes_gqa(B, Tn, H, H, D, splits);
}

// dt: 1 = bf16, 2 = fp16. qkv [B,Tn,(H+2*Hkv)*D]; kv [B,Tcap,2*Hkv*D]; pos = tokens already in the cache (host
// integer, the same for every batch row). Copies the K and V columns of qkv to cache rows [pos, pos+Tn).
// -1 = unsupported shape / dtype, Hkv < 1 or H % Hkv != 0, pos + Tn > Tcap, or operands not 16-byte aligned.
// shortfall: null, or int32 [B] on the device: row b is pos - shortfall[b] long instead of pos (clamped into
// [0, pos]) and its new rows go to [pos - shortfall[b], pos - shortfall[b] + Tn).
DL4J_API int dl4j_attn_kv_append_ragged_gqa_dt(int dt, const void* qkv, void* kv, const int* shortfall, int B, int Tn,
                                               int H, int Hkv, int D, int pos, int Tcap, hipStream_t s) {
  if (!decode_shape_ok(dt, B, Tn, H, Hkv, D, pos, Tcap) || !qkv || !kv) return -1;
  if (!attn_aligned16({qkv, kv})) return -1;
  const int EC = Hkv * D / 8, KC = H * D / 8, LDC = KC + 2 * EC;  // 16-byte chunks of Ekv / E / a source row
  const long long total = (long long)B * Tn * 2 * EC;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (shortfall)
    hipLaunchKernelGGL(attn_kv_append_ragged_kernel, grid, dim3(256), 0, s, (const uint4*)qkv, (uint4*)kv, total, Tn,
                       EC, LDC, KC, pos, Tcap, shortfall);
  else
    hipLaunchKernelGGL(attn_kv_append_kernel, grid, dim3(256), 0, s, (const uint4*)qkv, (uint4*)kv, total, Tn, EC, LDC,
                       KC, pos, Tcap);
  return (int)hipGetLastError();
}
DL4J_API int dl4j_attn_kv_append_ragged_dt(int dt, const void* qkv, void* kv, const int* shortfall, int B, int Tn,
                                           int H, int D, int pos, int Tcap, hipStream_t s) {
  return dl4j_attn_kv_append_ragged_gqa_dt(dt, qkv, kv, shortfall, B, Tn, H, H, D, pos, Tcap, s);
}

// Every batch row at pos.
DL4J_API int dl4j_attn_kv_append_gqa_dt(int dt, const void* qkv, void* kv, int B, int Tn, int H, int Hkv, int D,
                                        int pos, int Tcap, hipStream_t s) {
  return dl4j_attn_kv_append_ragged_gqa_dt(dt, qkv, kv, nullptr, B, Tn, H, Hkv, D, pos, Tcap, s);
}
DL4J_API int dl4j_attn_kv_append_dt(int dt, const void* qkv, void* kv, int B, int Tn, int H, int D, int pos, int Tcap,
                                    hipStream_t s) {
  return dl4j_attn_kv_append_ragged_gqa_dt(dt, qkv, kv, nullptr, B, Tn, H, H, D, pos, Tcap, s);
}

// The fp8 cache's append: kv8 [B,Tcap,R] bytes, R = 2*Hkv*D + roundup16(2*Hkv) (the layout at the top of this file);
// quantises the K and V columns of qkv into rows [pos, pos+Tn) (row b at pos - shortfall[b] with a shortfall array).
// Arguments and status codes of dl4j_attn_kv_append_ragged_gqa_dt.
DL4J_API int dl4j_attn_kv_append_fp8_ragged_gqa_dt(int dt, const void* qkv, void* kv8, const int* shortfall, int B,
                                                   int Tn, int H, int Hkv, int D, int pos, int Tcap, hipStream_t s) {
  if (!decode_shape_ok(dt, B, Tn, H, Hkv, D, pos, Tcap) || !qkv || !kv8) return -1;
  if (!attn_aligned16({qkv, kv8})) return -1;
  const long long total = (long long)B * Tn * 2 * Hkv * (D / 16);
  if ((total + 255) / 256 > 0x7fffffffLL) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    hipLaunchKernelGGL((attn_kv_append_fp8_kernel<DD, hb>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       (const hb*)qkv, (unsigned char*)kv8, total, Tn, Hkv, (H + 2 * Hkv) * DD, H * DD, pos, Tcap,
                       shortfall);
    return (int)hipGetLastError();
  });
}
DL4J_API int dl4j_attn_kv_append_fp8_ragged_dt(int dt, const void* qkv, void* kv8, const int* shortfall, int B, int Tn,
                                               int H, int D, int pos, int Tcap, hipStream_t s) {
  return dl4j_attn_kv_append_fp8_ragged_gqa_dt(dt, qkv, kv8, shortfall, B, Tn, H, H, D, pos, Tcap, s);
}

// Every batch row at pos.
DL4J_API int dl4j_attn_kv_append_fp8_gqa_dt(int dt, const void* qkv, void* kv8, int B, int Tn, int H, int Hkv, int D,
                                            int pos, int Tcap, hipStream_t s) {
  return dl4j_attn_kv_append_fp8_ragged_gqa_dt(dt, qkv, kv8, nullptr, B, Tn, H, Hkv, D, pos, Tcap, s);
}
DL4J_API int dl4j_attn_kv_append_fp8_dt(int dt, const void* qkv, void* kv8, int B, int Tn, int H, int D, int pos,
                                        int Tcap, hipStream_t s) {
  return dl4j_attn_kv_append_fp8_ragged_gqa_dt(dt, qkv, kv8, nullptr, B, Tn, H, H, D, pos, Tcap, s);
}

// The decode launch of all eight variants: FP8 picks the cache policy, Hkv == H the multi-head kernels.
template <bool FP8>
static int decode_launch(int dt, const void* qkv, const void* kv, void* out, float* ws, const int* shortfall, int B,
                         int Tn, int H, int Hkv, int D, int pos, int Tcap, int splits, float scale, hipStream_t s) {
  if (!decode_shape_ok(dt, B, Tn, H, Hkv, D, pos, Tcap) || !qkv || !kv || !out || splits < 1) return -1;
  if (!attn_aligned16({qkv, kv, out, ws})) return -1;
  const int S = decode_clamp_splits(splits, pos + Tn);
  if (S > 1 && !ws) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    using CP = std::conditional_t<FP8, KvCacheFp8<DD, hb>, KvCache16<DD, hb>>;
    using ce = typename CP::elem;
    const float scale2 = scale * kLog2e;
    if (Hkv != H) {
      const dim3 grid(S, B * Hkv, (Tn * (H / Hkv) + BLK - 1) / BLK);
      hipLaunchKernelGGL((attn_decode_gqa_kernel<DD, hb, CP>), grid, dim3(256), 0, s, (const hb*)qkv, (const ce*)kv,
                         (hb*)out, ws, Tn, H, Hkv, pos, Tcap, S, scale2, shortfall);
    } else {
      const dim3 grid(S, B * H, (Tn + BLK - 1) / BLK);
      if constexpr (FP8) {
        if (shortfall)
          hipLaunchKernelGGL((attn_decode_fp8_ragged_kernel<DD, hb>), grid, dim3(256), 0, s, (const hb*)qkv,
                             (const ce*)kv, (hb*)out, ws, Tn, H, pos, Tcap, S, scale2, shortfall);
        else
          hipLaunchKernelGGL((attn_decode_fp8_kernel<DD, hb>), grid, dim3(256), 0, s, (const hb*)qkv, (const ce*)kv,
                             (hb*)out, ws, Tn, H, pos, Tcap, S, scale2);
      } else {
        if (shortfall)
          hipLaunchKernelGGL((attn_decode_ragged_kernel<DD, hb>), grid, dim3(256), 0, s, (const hb*)qkv, (const ce*)kv,
                             (hb*)out, ws, Tn, H, pos, Tcap, S, scale2, shortfall);
        else
          hipLaunchKernelGGL((attn_decode_kernel<DD, hb>), grid, dim3(256), 0, s, (const hb*)qkv, (const ce*)kv,
                             (hb*)out, ws, Tn, H, pos, Tcap, S, scale2);
      }
    }
    if (S > 1) {
      const long long n = (long long)B * H * Tn * (DD / 4);
      hipLaunchKernelGGL((attn_decode_combine_kernel<DD, hb>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws,
                         (hb*)out, (long long)B * H, Tn, H, S);
    }
    return (int)hipGetLastError();
  });
}

// The windowed launch: the S splits divide the key blocks from the first one the window reaches (at the upper bound
// pos) to the last, so splits is clamped to that count.
template <bool FP8>
static int decode_win_launch(int dt, const void* qkv, const void* kv, void* out, float* ws, const int* shortfall,
                             int B, int Tn, int H, int Hkv, int D, int pos, int Tcap, int window, int splits,
                             float scale, hipStream_t s) {
  if (!decode_shape_ok(dt, B, Tn, H, Hkv, D, pos, Tcap) || !qkv || !kv || !out || splits < 1 || window < 1) return -1;
  if (!attn_aligned16({qkv, kv, out, ws})) return -1;
  const int W = window < pos + Tn ? window : pos + Tn;           // a wider window sees what pos + Tn sees
  const int first = (pos - W + 1 > 0 ? pos - W + 1 : 0) / BLK * BLK;
  const int S = decode_clamp_splits(splits, pos + Tn - first);
  if (S > 1 && !ws) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    using CP = std::conditional_t<FP8, KvCacheFp8<DD, hb>, KvCache16<DD, hb>>;
    using ce = typename CP::elem;
    const float scale2 = scale * kLog2e;
    const dim3 grid(S, B * Hkv, (Tn * (H / Hkv) + BLK - 1) / BLK);
    if (Hkv != H)
      hipLaunchKernelGGL((attn_decode_win_kernel<DD, hb, CP, true>), grid, dim3(256), 0, s, (const hb*)qkv,
                         (const ce*)kv, (hb*)out, ws, Tn, H, Hkv, pos, Tcap, S, scale2, W, shortfall);
    else
      hipLaunchKernelGGL((attn_decode_win_kernel<DD, hb, CP, false>), grid, dim3(256), 0, s, (const hb*)qkv,
                         (const ce*)kv, (hb*)out, ws, Tn, H, Hkv, pos, Tcap, S, scale2, W, shortfall);
    if (S > 1) {
      const long long n = (long long)B * H * Tn * (DD / 4);
      hipLaunchKernelGGL((attn_decode_combine_kernel<DD, hb>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws,
                         (hb*)out, (long long)B * H, Tn, H, S);
    }
    return (int)hipGetLastError();
  });
}

// out [B,Tn,H*D]; rows [0, pos+Tn) of kv [B,Tcap,2*Hkv*D] are the keys / values (the new rows already appended), query
// i sees keys <= pos + i. splits >= 1 is clamped to the number of 64-key blocks; ws: fp32 workspace of
// dl4j_attn_decode_ws_bytes_gqa(..., splits) bytes (may be null for one split). -1 = unsupported shape / dtype,
// Hkv < 1, H % Hkv != 0 or operands not 16-byte aligned.
// shortfall: null, or int32 [B] on the device: the keys of row b are rows [0, pos - shortfall[b] + Tn) and its query i
// sees keys <= pos - shortfall[b] + i. The grid and the split count still follow the upper bound pos.
DL4J_API int dl4j_attn_decode_ragged_gqa_dt(int dt, const void* qkv, const void* kv, void* out, float* ws,
                                            const int* shortfall, int B, int Tn, int H, int Hkv, int D, int pos,
                                            int Tcap, int splits, float scale, hipStream_t s) {
  return decode_launch<false>(dt, qkv, kv, out, ws, shortfall, B, Tn, H, Hkv, D, pos, Tcap, splits, scale, s);
}
DL4J_API int dl4j_attn_decode_ragged_dt(int dt, const void* qkv, const void* kv, void* out, float* ws,
                                        const int* shortfall, int B, int Tn, int H, int D, int pos, int Tcap,
                                        int splits, float scale, hipStream_t s) {
  return decode_launch<false>(dt, qkv, kv, out, ws, shortfall, B, Tn, H, H, D, pos, Tcap, splits, scale, s);
}

// Every batch row at pos.
DL4J_API int dl4j_attn_decode_gqa_dt(int dt, const void* qkv, const void* kv, void* out, float* ws, int B, int Tn,
                                     int H, int Hkv, int D, int pos, int Tcap, int splits, float scale,
                                     hipStream_t s) {
  return decode_launch<false>(dt, qkv, kv, out, ws, nullptr, B, Tn, H, Hkv, D, pos, Tcap, splits, scale, s);
}
DL4J_API int dl4j_attn_decode_dt(int dt, const void* qkv, const void* kv, void* out, float* ws, int B, int Tn, int H,
                                 int D, int pos, int Tcap, int splits, float scale, hipStream_t s) {
  return decode_launch<false>(dt, qkv, kv, out, ws, nullptr, B, Tn, H, H, D, pos, Tcap, splits, scale, s);
}

// The same over the fp8 cache kv8 [B,Tcap,R] bytes: the same arguments, split clamp, workspace and status codes; for
// a given split count the result is bitwise what the 16-bit entry gives on the dequantised cache.
DL4J_API int dl4j_attn_decode_fp8_ragged_gqa_dt(int dt, const void* qkv, const void* kv8, void* out, float* ws,
                                                const int* shortfall, int B, int Tn, int H, int Hkv, int D, int pos,
                                                int Tcap, int splits, float scale, hipStream_t s) {
  return decode_launch<true>(dt, qkv, kv8, out, ws, shortfall, B, Tn, H, Hkv, D, pos, Tcap, splits, scale, s);
}
DL4J_API int dl4j_attn_decode_fp8_ragged_dt(int dt, const void* qkv, const void* kv8, void* out, float* ws,
                                            const int* shortfall, int B, int Tn, int H, int D, int pos, int Tcap,
                                            int splits, float scale, hipStream_t s) {
  return decode_launch<true>(dt, qkv, kv8, out, ws, shortfall, B, Tn, H, H, D, pos, Tcap, splits, scale, s);
}

// Every batch row at pos.
DL4J_API int dl4j_attn_decode_fp8_gqa_dt(int dt, const void* qkv, const void* kv8, void* out, float* ws, int B, int Tn,
                                         int H, int Hkv, int D, int pos, int Tcap, int splits, float scale,
                                         hipStream_t s) {
  return decode_launch<true>(dt, qkv, kv8, out, ws, nullptr, B, Tn, H, Hkv, D, pos, Tcap, splits, scale, s);
}
DL4J_API int dl4j_attn_decode_fp8_dt(int dt, const void* qkv, const void* kv8, void* out, float* ws, int B, int Tn,
                                     int H, int D, int pos, int Tcap, int splits, float scale, hipStream_t s) {
  return decode_launch<true>(dt, qkv, kv8, out, ws, nullptr, B, Tn, H, H, D, pos, Tcap, splits, scale, s);
}

// Cached decoding with a sliding window: query i sees keys pos + i - window < k <= pos + i (at pos - shortfall[b] in a
// ragged batch). Arguments, workspace and status codes of dl4j_attn_decode_ragged_gqa_dt (shortfall may be null,
// Hkv = H is plain multi-head); -1 also for window < 1. The key blocks wholly before the window are not read, and
// splits divides (and is clamped to) the blocks from the first one the window reaches at pos to the last: size it
// with dl4j_attn_decode_splits_gqa on that many keys, not on pos + Tn. window >= pos + Tn gives the bits of the
// unwindowed entry at the same split count.
DL4J_API int dl4j_attn_decode_win_dt(int dt, const void* qkv, const void* kv, void* out, float* ws,
                                     const int* shortfall, int B, int Tn, int H, int Hkv, int D, int pos, int Tcap,
                                     int window, int splits, float scale, hipStream_t s) {
  return decode_win_launch<false>(dt, qkv, kv, out, ws, shortfall, B, Tn, H, Hkv, D, pos, Tcap, window, splits, scale,
                                  s);
}

// The same over the fp8 cache kv8 [B,Tcap,R] bytes.
DL4J_API int dl4j_attn_decode_win_fp8_dt(int dt, const void* qkv, const void* kv8, void* out, float* ws,
                                         const int* shortfall, int B, int Tn, int H, int Hkv, int D, int pos,
                                         int Tcap, int window, int splits, float scale, hipStream_t s) {
  return decode_win_launch<true>(dt, qkv, kv8, out, ws, shortfall, B, Tn, H, Hkv, D, pos, Tcap, window, splits, scale,
                                 s);
}
