// Weight-only MXFP8 / MXFP4 products for decoding: out[M, N] = act(x[M, K] · deq(Wq) + bias + beta·out), M <= 64.
//
// Format (OCP microscaling): W [K, N] is quantised in groups of 32 consecutive k per output column, one E8M0 scale
// byte `ex + 127` per group and 32 codes, e4m3fn (BITS 8) or e2m1 (BITS 4). ex is the smallest exponent with
// max|w| * 2^-ex <= 448 (6), codes round to nearest even and saturate, an all-zero group has ex = 0. value =
// code * 2^ex, exact in bf16 / fp16.
//
// Packed layout, chosen so that one 16-byte load per lane IS the lane's MFMA operand fragments:
//   a tile is CW = 16 * CT columns (CT = 8 / BITS column fragments: 1 for fp8, 2 for fp4) x 64 k (two groups) and
//   1024 bytes: lane l = 16 q + c of a wave owns bytes [16 l, 16 l + 16) =
//     fp8: [j][i]        code of column c,           k = 64 kt + 32 j + 8 q + i       (j < 2, i < 8)
//     fp4: [ct][j][p]    codes of column 16 ct + c,  k = .. + 2 p (low nibble), 2 p + 1 (high nibble)   (p < 4)
//   i.e. for v_mfma_f32_16x16x32 with the weights on the 16-wide row side, lane (q, c) holds row c, k = 8 q .. 8 q + 7
//   of the 32-deep step j. Tiles are stored [column block nb][kt], so a block streams contiguous memory along K.
//   Scales: [nb][kt][c][ct][j] bytes, the CT * 2 bytes a lane needs in one 2- / 4-byte load.
//   K is padded to 64 and N to CW with zero codes and scale byte 127.
//
// dl4j_wq_gemm: a block of 4 waves owns ONE column block (16 / 32 output columns) and a range of 256-deep K chunks;
// wave w takes tile 4 ch + w of every chunk ch, so the four waves split K inside the block. Weight bytes go global ->
// registers (one dwordx4 per lane per tile, every byte read once chip-wide), are converted in registers
// (v_cvt_scalef32_pk_{bf16,f16}_{fp8,fp4}, the scale byte placed into an fp32 exponent) and feed the MFMA as the
// row-side operand; the column side is x, so M <= 16 / 32 / 64 costs MF = 1 / 2 / 4 column fragments and no padding
// rows of weights are ever multiplied. The x chunk [16 MF, 256] is staged in LDS once per block (row pitch 264: the 16
// rows of a fragment read land on distinct banks) and read by all four waves. The waves' accumulators are summed in
// wave order through the same LDS. When the column blocks alone do not cover the chip the grid splits K further
// (blockIdx.y); those partials go to an fp32 workspace [S][M][Np] and dl4j's merge launch sums them in split order and
// applies the epilogue: no float atomics anywhere, two runs give the same bits. The launch geometry depends on
// (bits, M, N, K) only and nothing is read back.
//
// dl4j_wq_gemm_grouped: the same block for the experts of a mixture-of-experts step of Ntok <= 64 tokens. The X packed
// matrices lie one after another; the grid is (column blocks, X, S). Block (nb, e, s) reads cnt[e] / off[e] of the
// routing plan (csrc/moe.hip) on the device: an expert without assignments leaves before its first weight load, the
// others multiply only the first ceil(cnt[e] / 16) of the MF = ceil(Ntok / 16) column fragments (a token's experts are
// distinct, so cnt[e] <= Ntok). Panel row r is either gathered, x[src_of[off[e] + r] / k] of the token-major
// activations (no gathered copy and no gather launch), or row off[e] + r of an expert-sorted buffer; rows from cnt[e]
// on are zeros. Output row off[e] + r of the expert-sorted buffer, live rows only. Split-K partials are kept for live
// rows only, [S][Ntok * k][Np] at the compact row (exclusive prefix of cnt)[e] + r, and merged in split order.
//
// The epilogue, the split-K partial layout and merge launches, the routing-plan prelude of the grouped product, the
// split rule and the operand checks are csrc/skinny_body.h's, shared with csrc/gemm_skinny.hip.
#include "skinny_body.h"

namespace {

constexpr int WQ_KT = 64;        // k per tile
constexpr int WQ_KC = 256;       // k per chunk: one tile per wave
constexpr int WQ_LDX = WQ_KC + 8;

__device__ __forceinline__ float wq_scale(unsigned byte) { return __uint_as_float(byte << 23); }

// 8 codes -> the fragment: fp8 from two dwords, fp4 from one
__device__ __forceinline__ SV8<__bf16> wq_deq8(unsigned a, unsigned b, float sc, __bf16) {
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, false);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, sc, true);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, false);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, sc, true);
  return SV8<__bf16>{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
__device__ __forceinline__ SV8<_Float16> wq_deq8(unsigned a, unsigned b, float sc, _Float16) {
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(a, sc, false);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(a, sc, true);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(b, sc, false);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(b, sc, true);
  return SV8<_Float16>{(_Float16)p0[0], (_Float16)p0[1], (_Float16)p1[0], (_Float16)p1[1],
                       (_Float16)p2[0], (_Float16)p2[1], (_Float16)p3[0], (_Float16)p3[1]};
}
__device__ __forceinline__ SV8<__bf16> wq_deq4(unsigned a, float sc, __bf16) {
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 0);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 1);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 2);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 3);
  return SV8<__bf16>{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
__device__ __forceinline__ SV8<_Float16> wq_deq4(unsigned a, float sc, _Float16) {
  const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(a, sc, 0);
  const auto p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(a, sc, 1);
  const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(a, sc, 2);
  const auto p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(a, sc, 3);
  return SV8<_Float16>{(_Float16)p0[0], (_Float16)p0[1], (_Float16)p1[0], (_Float16)p1[1],
                       (_Float16)p2[0], (_Float16)p2[1], (_Float16)p3[0], (_Float16)p3[1]};
}

// The code format as a policy of the one GEMM / quantise / dequantise body.
template <int BITS> struct WqFmt;
template <> struct WqFmt<8> {
  static constexpr int CT = 1;
  // fragment (ct, j) of the lane's 16 bytes w and its scale bytes sc
  template <typename hb> static __device__ __forceinline__ SV8<hb> frag(const uint4& w, unsigned sc, int, int j) {
    const float s = wq_scale((sc >> (8 * j)) & 0xffu);
    return j == 0 ? wq_deq8(w.x, w.y, s, hb()) : wq_deq8(w.z, w.w, s, hb());
  }
  static __device__ __forceinline__ unsigned load_scales(const unsigned char* p) {
    return *reinterpret_cast<const unsigned short*>(p);
  }
  // ex of a group from its largest magnitude: 448 = 0.875 * 2^9
  static __device__ __forceinline__ int exponent(float amax) {
    int e;
    const float m = frexpf(amax, &e);
    return m <= 0.875f ? e - 9 : e - 8;
  }
  // 8 values of one group -> dwords d[0], d[1]
  static __device__ __forceinline__ void encode(const float* x, int ex, unsigned* d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int v = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x[4 * h], -ex), ldexpf(x[4 * h + 1], -ex), 0, false);
      v = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x[4 * h + 2], -ex), ldexpf(x[4 * h + 3], -ex), v, true);
      d[h] = (unsigned)v;
    }
  }
};
template <> struct WqFmt<4> {
  static constexpr int CT = 2;
  template <typename hb> static __device__ __forceinline__ SV8<hb> frag(const uint4& w, unsigned sc, int ct, int j) {
    const int i = ct * 2 + j;
    const float s = wq_scale((sc >> (8 * i)) & 0xffu);
    const unsigned d = i == 0 ? w.x : (i == 1 ? w.y : (i == 2 ? w.z : w.w));
    return wq_deq4(d, s, hb());
  }
  static __device__ __forceinline__ unsigned load_scales(const unsigned char* p) {
    return *reinterpret_cast<const unsigned*>(p);
  }
  // 6 = 0.75 * 2^3
  static __device__ __forceinline__ int exponent(float amax) {
    int e;
    const float m = frexpf(amax, &e);
    return m <= 0.75f ? e - 3 : e - 2;
  }
  // 8 values of one group -> one dword d[0]
  static __device__ __forceinline__ void encode(const float* x, int ex, unsigned* d) {
    const float s = __uint_as_float((unsigned)(ex + 127) << 23);
    unsigned v = 0;
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, x[0], x[1], s, 0);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, x[2], x[3], s, 1);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, x[4], x[5], s, 2);
    v = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(v, x[6], x[7], s, 3);
    d[0] = v;
  }
};

// The K loop of one block and the waves' sum in wave order: tail(s, m, n) receives the block's sums for panel row m
// and columns n .. n + 3, for every row of the live fragments. src(r): the x row of panel row r or -1 for zeros; mfl:
// the live fragments (block-uniform). xs: the x panel [16 MF, WQ_LDX], reused for the wave reduction.
template <int BITS, typename hb, int MF, typename Src, typename Tail>
__device__ __forceinline__ void wq_block(const uint4* __restrict__ codes, const unsigned char* __restrict__ scales,
                                         const hb* __restrict__ x, int ldx, Src src, int mfl, int K, int KTn, int nb,
                                         int ch0, int ch1, hb* xs, Tail tail) {
  using F = WqFmt<BITS>;
  constexpr int CT = F::CT, CW = 16 * CT;
  static_assert(sizeof(hb) * MF * 16 * WQ_LDX >= 4 * CT * MF * 64 * sizeof(sk_f4), "reduction fits the x panel");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  sk_f4 acc[CT][MF];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int f = 0; f < MF; ++f) acc[ct][f] = sk_f4{0.f, 0.f, 0.f, 0.f};

  for (int ch = ch0; ch < ch1; ++ch) {
    const int kt = ch * 4 + wave;
    const bool live = kt < KTn;                                        // wave-uniform
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    unsigned sc = 0x7f7f7f7fu;
    if (live) {
      const long long tile = (long long)nb * KTn + kt;
      w = codes[tile * 64 + lane];
      sc = F::load_scales(scales + (tile * 16 + c) * (CT * 2));
    }
    __syncthreads();                                                   // the previous chunk's fragment reads are done
    const int kc = ch * WQ_KC;
    for (int i = tid; i < mfl * 16 * (WQ_KC / 8); i += 256) {
      const int r = i >> 5, k8 = (i & 31) * 8;
      const int sr = src(r);
      SV8<hb> v = SV8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
      if (sr >= 0 && kc + k8 < K) v = *reinterpret_cast<const SV8<hb>*>(x + (long long)sr * ldx + kc + k8);
      *reinterpret_cast<SV8<hb>*>(xs + r * WQ_LDX + k8) = v;
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int koff = wave * WQ_KT + j * 32 + q * 8;
        SV8<hb> b[MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) {
          b[f] = SV8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
          if (f < mfl) b[f] = *reinterpret_cast<const SV8<hb>*>(xs + (f * 16 + c) * WQ_LDX + koff);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const SV8<hb> a = F::template frag<hb>(w, sc, ct, j);
#pragma unroll
          for (int f = 0; f < MF; ++f)
            if (f < mfl) acc[ct][f] = sk_mma(a, b[f], acc[ct][f]);     // block-uniform: dead fragments cost nothing
        }
      }
    }
  }
  // the four waves' sums, in wave order
  __syncthreads();
  sk_f4* red = reinterpret_cast<sk_f4*>(xs);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int f = 0; f < MF; ++f) red[((wave * CT + ct) * MF + f) * 64 + lane] = acc[ct][f];
  __syncthreads();
  for (int idx = tid; idx < CT * mfl * 64; idx += 256) {
    const int l = idx & 63, f = (idx >> 6) % mfl, ct = (idx >> 6) / mfl;
    sk_f4 s = red[((0 * CT + ct) * MF + f) * 64 + l];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) s += red[((wv * CT + ct) * MF + f) * 64 + l];
    tail(s, f * 16 + (l & 15), nb * CW + ct * 16 + 4 * (l >> 4));
  }
}

template <int BITS, typename hb, int MF>
__global__ __launch_bounds__(256) void wq_gemm_kernel(const uint4* __restrict__ codes,
                                                      const unsigned char* __restrict__ scales,
                                                      const hb* __restrict__ x, int ldx, int M, int N, int K, int KTn,
                                                      int cpb, float* __restrict__ ws, SkEpi epi) {
  __shared__ __attribute__((aligned(16))) hb xs[MF * 16 * WQ_LDX];
  const int NC = (KTn + 3) >> 2;
  const int ch0 = blockIdx.y * cpb, ch1 = min(NC, ch0 + cpb);
  const int Np = gridDim.x * 16 * WqFmt<BITS>::CT;
  wq_block<BITS, hb, MF>(codes, scales, x, ldx, [M](int r) { return r < M ? r : -1; }, MF, K, KTn, blockIdx.x, ch0,
                         ch1, xs, [&](sk_f4 s, int m, int n) {
                           if (m >= M) return;
                           if (gridDim.y > 1) *reinterpret_cast<sk_f4*>(sk_partial(ws, blockIdx.y, M, m, Np, n)) = s;
                           else sk_epilogue4<hb>(epi, s, m, n, N);
                         });
}

// Block (nb, e, s) of the grouped product: wq_gemm_kernel's body on expert e's packed matrix, over the expert's live
// rows only.
template <int BITS, typename hb, int MF, bool GATHER>
__global__ __launch_bounds__(256) void wq_gemm_grouped_kernel(const uint4* __restrict__ codes,
                                                              const unsigned char* __restrict__ scales,
                                                              long long cstride, long long sstride,
                                                              const hb* __restrict__ x, int ldx, SkPlan p, int N, int K,
                                                              int KTn, int cpb, float* __restrict__ ws, SkEpi epi) {
  __shared__ __attribute__((aligned(16))) hb xs[MF * 16 * WQ_LDX];
  __shared__ int rowsrc[MF * 16];                                          // the x row of panel row r, -1: zeros
  const int e = blockIdx.y;
  const SkGroup g = sk_group<MF>(p, e);
  if (g.rows <= 0) return;                                                 // block-uniform: no byte of an idle expert
  sk_group_rows<MF, GATHER>(p, g, rowsrc);
  const int NC = (KTn + 3) >> 2;
  const int ch0 = blockIdx.z * cpb, ch1 = min(NC, ch0 + cpb);
  const int Np = gridDim.x * 16 * WqFmt<BITS>::CT;
  const int pre = gridDim.z > 1 ? sk_group_pre(p, e) : 0;
  const SkEpi le = sk_expert_epi(epi, e, N);
  // rowsrc is read behind the body's first barrier
  wq_block<BITS, hb, MF>(codes + (long long)e * cstride, scales + (long long)e * sstride, x, ldx,
                         [&](int r) { return rowsrc[r]; }, g.mfl, K, KTn, blockIdx.x, ch0, ch1, xs,
                         [&](sk_f4 s, int m, int n) {
                           if (m >= g.rows) return;
                           const int cr = pre + m;                         // the compact row
                           if (gridDim.z == 1) sk_epilogue4<hb>(le, s, g.off + m, n, N);
                           else if (cr >= 0 && cr < p.A)
                             *reinterpret_cast<sk_f4*>(sk_partial(ws, blockIdx.z, p.A, cr, Np, n)) = s;
                         });
}

// One wave per tile (nb, kt): W [K, N] with element strides (sk, sn) -> the tile's 1024 code bytes and scale bytes.
// A group's 32 values sit in the four lanes q = 0..3 of a column c: its maximum is two cross-lane exchanges.
template <int BITS, typename hb>
__global__ __launch_bounds__(256) void wq_quantize_kernel(const hb* __restrict__ W, long long sk, long long sn, int K,
                                                          int N, int KTn, long long tiles, uint4* __restrict__ codes,
                                                          unsigned char* __restrict__ scales) {
  using F = WqFmt<BITS>;
  constexpr int CT = F::CT, CW = 16 * CT;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= tiles) return;
  const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const int nb = (int)(tile / KTn), kt = (int)(tile - (long long)nb * KTn);
  unsigned d[4] = {0u, 0u, 0u, 0u};
  unsigned sb = 0;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = nb * CW + ct * 16 + c;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k0 = kt * WQ_KT + j * 32 + q * 8;
      float x[8];
      float amax = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        x[i] = (n < N && k0 + i < K) ? (float)W[(long long)(k0 + i) * sk + (long long)n * sn] : 0.f;
        amax = fmaxf(amax, fabsf(x[i]));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      int ex = amax > 0.f ? F::exponent(amax) : 0;
      ex = min(max(ex, -126), 127);
      F::encode(x, ex, d + (BITS == 8 ? 2 * j : ct * 2 + j));
      sb |= (unsigned)(ex + 127) << (8 * (ct * 2 + j));
    }
  }
  codes[tile * 64 + lane] = make_uint4(d[0], d[1], d[2], d[3]);
  if (q == 0) {
    unsigned char* sp = scales + (tile * 16 + c) * (CT * 2);
    if (CT == 1) *reinterpret_cast<unsigned short*>(sp) = (unsigned short)sb;
    else *reinterpret_cast<unsigned*>(sp) = sb;
  }
}

// One wave per tile: packed -> out [K, N] (row-major, 16-bit): the values the GEMM's fragments hold.
template <int BITS, typename hb>
__global__ __launch_bounds__(256) void wq_dequant_kernel(const uint4* __restrict__ codes,
                                                         const unsigned char* __restrict__ scales, int K, int N,
                                                         int KTn, long long tiles, hb* __restrict__ out) {
  using F = WqFmt<BITS>;
  constexpr int CT = F::CT, CW = 16 * CT;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= tiles) return;
  const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const int nb = (int)(tile / KTn), kt = (int)(tile - (long long)nb * KTn);
  const uint4 w = codes[tile * 64 + lane];
  const unsigned sc = F::load_scales(scales + (tile * 16 + c) * (CT * 2));
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = nb * CW + ct * 16 + c;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const SV8<hb> v = F::template frag<hb>(w, sc, ct, j);
      const int k0 = kt * WQ_KT + j * 32 + q * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (k0 + i < K) out[(long long)(k0 + i) * N + n] = v[i];
    }
  }
}

inline int wq_cw(int bits) { return bits == 8 ? 16 : 32; }
inline bool wq_shape_ok(int bits, long long K, long long N) {
  return (bits == 8 || bits == 4) && K >= 32 && K % 32 == 0 && N >= 1 && K <= (1 << 24) && N <= (1 << 24);
}

// split count and chunks per block from (bits, M, N, K) alone: sk_split_plan on this format's column blocks and the
// 256-deep chunks (one 64-deep tile per wave)
inline void wq_split(int bits, int M, int N, int K, int* S, int* cpb) {
  sk_split_plan(wq_cw(bits), WQ_KC, bits, M, N, K, S, cpb);
}
// wq_split for the grouped product, from (bits, Ntok, k, X, N, K) alone
inline void wq_split_grouped(int bits, int Ntok, int k, int X, int N, int K, int* S, int* cpb) {
  sk_split_plan_grouped(wq_cw(bits), WQ_KC, bits, Ntok, k, X, N, K, S, cpb);
}

inline bool wq_grouped_ok(int bits, int Ntok, int k, int X, long long N, long long K) {
  return wq_shape_ok(bits, K, N) && sk_routing_ok(Ntok, k, X);
}

}  // namespace

// Bytes of the packed codes and of the scales of W [K, N] in format `bits` (8 / 4); -1: a shape the format refuses
// (K % 32 != 0, bits).
DL4J_API int dl4j_wq_packed_bytes(int bits, long long K, long long N, long long* code_bytes, long long* scale_bytes) {
  if (!wq_shape_ok(bits, K, N) || !code_bytes || !scale_bytes) return -1;
  const long long nbk = (N + wq_cw(bits) - 1) / wq_cw(bits), KTn = (K + WQ_KT - 1) / WQ_KT;
  *code_bytes = nbk * KTn * 1024;
  *scale_bytes = nbk * KTn * 16 * (bits == 8 ? 2 : 4);
  return 0;
}

// W [K, N] (dtype 1 bf16 / 2 fp16, element strides sk, sn) -> codes, scales (16-byte aligned, dl4j_wq_packed_bytes).
DL4J_API int dl4j_wq_quantize(int bits, int dtype, const void* W, long long sk, long long sn, long long K, long long N,
                              void* codes, void* scales, hipStream_t s) {
  if (!wq_shape_ok(bits, K, N) || !W || !sk_al16(codes) || !sk_al16(scales) || (dtype != 1 && dtype != 2)) return -1;
  const int KTn = (int)((K + WQ_KT - 1) / WQ_KT);
  const long long tiles = (N + wq_cw(bits) - 1) / wq_cw(bits) * KTn;
  const dim3 grid((unsigned)((tiles + 3) / 4));
#define L(B, T) hipLaunchKernelGGL((wq_quantize_kernel<B, T>), grid, dim3(256), 0, s, (const T*)W, sk, sn, (int)K, \
                                   (int)N, KTn, tiles, (uint4*)codes, (unsigned char*)scales)
  if (bits == 8 && dtype == 1) L(8, __bf16);
  else if (bits == 8) L(8, _Float16);
  else if (dtype == 1) L(4, __bf16);
  else L(4, _Float16);
#undef L
  return (int)hipGetLastError();
}

// packed -> out [K, N] contiguous in dtype (1 bf16 / 2 fp16).
DL4J_API int dl4j_wq_dequant(int bits, int dtype, const void* codes, const void* scales, long long K, long long N,
                             void* out, hipStream_t s) {
  if (!wq_shape_ok(bits, K, N) || !out || !sk_al16(codes) || !sk_al16(scales) || (dtype != 1 && dtype != 2)) return -1;
  const int KTn = (int)((K + WQ_KT - 1) / WQ_KT);
  const long long tiles = (N + wq_cw(bits) - 1) / wq_cw(bits) * KTn;
  const dim3 grid((unsigned)((tiles + 3) / 4));
#define L(B, T) hipLaunchKernelGGL((wq_dequant_kernel<B, T>), grid, dim3(256), 0, s, (const uint4*)codes, \
                                   (const unsigned char*)scales, (int)K, (int)N, KTn, tiles, (T*)out)
  if (bits == 8 && dtype == 1) L(8, __bf16);
  else if (bits == 8) L(8, _Float16);
  else if (dtype == 1) L(4, __bf16);
  else L(4, _Float16);
#undef L
  return (int)hipGetLastError();
}

// Floats of split-K workspace dl4j_wq_gemm needs for (bits, M, N, K): 0 when the product runs unsplit, -1 for a shape
// it refuses.
DL4J_API long long dl4j_wq_gemm_workspace(int bits, int M, long long N, long long K) {
  if (!wq_shape_ok(bits, K, N) || M < 1 || M > 64) return -1;
  int S, cpb;
  wq_split(bits, M, (int)N, (int)K, &S, &cpb);
  return sk_ws_floats(S, M, N, wq_cw(bits));
}

// out [M, ldo] = act(x [M, ldx] · deq(codes, scales) + bias + beta·out), 1 <= M <= 64. dtype 1 bf16 / 2 fp16 (x and
// out); bias [N] of dtype bias_dt (0 fp32, 1, 2) or null; beta 0 / 1; act 0 none / 4 GELU; ws: the floats
// dl4j_wq_gemm_workspace asks for (may be null when 0). -1: refused (shape, alignment, dtype), nothing launched.
DL4J_API int dl4j_wq_gemm(int bits, int dtype, const void* x, long long ldx, int M, long long N, long long K,
                          const void* codes, const void* scales, void* out, long long ldo, const void* bias,
                          int bias_dt, int beta, int act, void* ws, hipStream_t s) {
  if (!wq_shape_ok(bits, K, N) || !sk_dense_ok(M, beta, bias_dt) || !sk_operands_ok(dtype, x, ldx, K, out, ldo, N, act))
    return -1;
  if (!sk_al16(codes) || !sk_al16(scales)) return -1;
  int S, cpb;
  wq_split(bits, M, (int)N, (int)K, &S, &cpb);
  if (S > 1 && !sk_al16(ws)) return -1;
  const int KTn = (int)((K + WQ_KT - 1) / WQ_KT), cw = wq_cw(bits);
  const int nbk = (int)((N + cw - 1) / cw);
  const SkEpi epi{out, bias, (int)ldo, bias_dt, beta, act};
  const dim3 grid((unsigned)nbk, (unsigned)S);
  const int mf = sk_mf(M);
#define L(B, T, F) hipLaunchKernelGGL((wq_gemm_kernel<B, T, F>), grid, dim3(256), 0, s, (const uint4*)codes,      \
                                      (const unsigned char*)scales, (const T*)x, (int)ldx, M, (int)N, (int)K, KTn, \
                                      cpb, (float*)ws, epi)
#define LM(B, T) do { if (mf == 1) L(B, T, 1); else if (mf == 2) L(B, T, 2); else L(B, T, 4); } while (0)
  if (bits == 8 && dtype == 1) LM(8, __bf16);
  else if (bits == 8) LM(8, _Float16);
  else if (dtype == 1) LM(4, __bf16);
  else LM(4, _Float16);
#undef LM
#undef L
  const int rc = (int)hipGetLastError();
  return rc != 0 || S == 1 ? rc : sk_merge(dtype, ws, S, M, (int)N, nbk * cw, epi, s);
}

// Floats of split-K workspace dl4j_wq_gemm_grouped needs for (bits, Ntok, k, X, N, K): 0 when the product runs
// unsplit, -1 for a shape it refuses.
DL4J_API long long dl4j_wq_gemm_grouped_workspace(int bits, int Ntok, int k, int X, long long N, long long K) {
  if (!wq_grouped_ok(bits, Ntok, k, X, N, K)) return -1;
  int S, cpb;
  wq_split_grouped(bits, Ntok, k, X, (int)N, (int)K, &S, &cpb);
  return sk_ws_floats(S, (long long)Ntok * k, N, wq_cw(bits));
}

// The experts' products of a mixture-of-experts step of Ntok <= 64 tokens on X packed matrices [K, N] (expert e's codes
// at codes + e * code_stride bytes, its scales at scales + e * scale_stride; strides multiples of 16, at least
// dl4j_wq_packed_bytes): out[off[e] + r] = act(row_r · deq(W_e) + bias[e]) for r < cnt[e], with cnt [X], off [X + 1]
// and src_of [Rcap] the plan of dl4j_moe_route for (Ntok, k, X). gather 1: row_r = x[src_of[off[e] + r] / k], x the
// token-major activations [Ntok, ldx]; gather 0: row_r = x[off[e] + r], x an expert-sorted buffer [Rcap, ldx] (src_of
// may be null). out [Rcap, ldo]: pad rows and the segments of idle experts are not written. dtype 1 bf16 / 2 fp16;
// bias fp32 [X, N] or null; act 0 none / 4 GELU; ws: the floats dl4j_wq_gemm_grouped_workspace asks for (may be null
// when 0). The plan is read on the device only. -1: refused (shape, Ntok > 64, alignment, dtype), nothing launched.
DL4J_API int dl4j_wq_gemm_grouped(int bits, int dtype, const void* x, long long ldx, int gather, int Ntok, int k, int X,
                                  long long Rcap, long long N, long long K, const void* codes, const void* scales,
                                  long long code_stride, long long scale_stride, const int* cnt, const int* off,
                                  const int* src_of, void* out, long long ldo, const float* bias, int act, void* ws,
                                  hipStream_t s) {
  if (!wq_grouped_ok(bits, Ntok, k, X, N, K) || !sk_operands_ok(dtype, x, ldx, K, out, ldo, N, act)) return -1;
  if (!sk_plan_ok(gather, Ntok, k, Rcap, cnt, off, src_of, bias) || !sk_al16(codes) || !sk_al16(scales)) return -1;
  long long cb, sb;
  dl4j_wq_packed_bytes(bits, K, N, &cb, &sb);
  if (code_stride < cb || code_stride % 16 || scale_stride < sb || scale_stride % 16) return -1;
  int S, cpb;
  wq_split_grouped(bits, Ntok, k, X, (int)N, (int)K, &S, &cpb);
  if (S > 1 && !sk_al16(ws)) return -1;
  const int KTn = (int)((K + WQ_KT - 1) / WQ_KT), cw = wq_cw(bits);
  const int nbk = (int)((N + cw - 1) / cw);
  const SkEpi epi{out, bias, (int)ldo, 0, 0, act};
  const SkPlan plan{cnt, off, src_of, Ntok, k, X, Ntok * k, Rcap};
  const dim3 grid((unsigned)nbk, (unsigned)X, (unsigned)S);
  const int mf = sk_mf(Ntok);
#define L(B, T, F, G) hipLaunchKernelGGL((wq_gemm_grouped_kernel<B, T, F, G>), grid, dim3(256), 0, s,                \
                                         (const uint4*)codes, (const unsigned char*)scales, code_stride / 16,        \
                                         scale_stride, (const T*)x, (int)ldx, plan, (int)N, (int)K, KTn, cpb,        \
                                         (float*)ws, epi)
#define LG(B, T, F) do { if (gather) L(B, T, F, true); else L(B, T, F, false); } while (0)
#define LM(B, T) do { if (mf == 1) LG(B, T, 1); else if (mf == 2) LG(B, T, 2); else LG(B, T, 4); } while (0)
  if (bits == 8 && dtype == 1) LM(8, __bf16);
  else if (bits == 8) LM(8, _Float16);
  else if (dtype == 1) LM(4, __bf16);
  else LM(4, _Float16);
#undef LM
#undef LG
#undef L
  const int rc = (int)hipGetLastError();
  return rc != 0 || S == 1 ? rc : sk_merge_grouped(dtype, ws, S, plan, (int)N, nbk * cw, epi, s);
}
