// Skinny 16-bit products for decoding: out[M, N] = act(x[M, K] · W[K, N] + bias + beta·out), M <= 64, on the bf16 /
// fp16 weights where they lie: no packed copy, no conversion. The weights sit on the 16-wide row side of
// v_mfma_f32_16x16x32_{bf16,f16} and x on the column side, so M <= 16 / 32 / 64 costs MF = 1 / 2 / 4 column fragments
// and no padding rows are multiplied (the shape of csrc/gemm_wq.hip's kernel).
//
// Three layouts of the weight operand, LAY:
//   0  K-contiguous (sk == 1, element (k, n) at W + n * ld + k: RnnOutputLayer.W). A column block is 16 columns; lane
//      (q, c) of a wave holds column n0 + c, k = k0 + 8 q .. 8 q + 7 of a 32-deep step: one 16-byte load IS the fragment.
//   1  N-contiguous (sn == 1, element (k, n) at W + k * ld + n: Wqkv, Wo, W1, W2, the stacked experts), 16-byte loads.
//      A column block is 128 columns. For a 32-deep step lane (q, c) loads the 8 rows k0 + 8 q + i (i < 8) of the 8
//      columns n0 + 8 c .. + 7 and the wave issues 8 MFMAs: in MFMA t the lane's operand is element t of each of its
//      8 vectors, gathered by four v_perm_b32, so MFMA row c stands for column n0 + 8 c + t. The matrix is turned in
//      registers; x is read from LDS in the same k order. Accumulator row 4 q + r of MFMA t is column
//      n0 + 32 q + 8 r + t: every lane ends with 32 consecutive columns of token c.
//   2  N-contiguous, 8-byte loads: 4 columns per lane, 64-column blocks, 4 MFMAs per step, 16 consecutive columns per
//      lane. Twice the column blocks for narrow N.
//
// A block of 4 waves owns one column block and a range of K chunks (256 deep for layout 0, 128 for 1 / 2); wave w
// takes the w-th quarter of every chunk. The next chunk's weights are loaded while the current one is multiplied. The
// x chunk [16 MF, chunk] is staged once per block in LDS (row pitch chunk + 8: the 16 rows of a fragment read land on
// distinct banks) and read by all four waves. The waves' accumulators are summed in wave order through the same LDS
// and wave 3 runs the epilogue from its registers, 4 / 32 / 16 consecutive columns per lane, as 16-byte vectors where
// the output is aligned. When the column blocks do not cover the chip the grid splits K further; those partials go to
// an fp32 workspace [S][M][Np] and a merge launch sums them in split order and applies the epilogue. No float atomics:
// two runs give the same bits. The launch geometry depends on (layout, M, N, K) alone and nothing is read back.
//
// K and N are free: rows from K on enter as zeros (never loaded), tail columns are masked, a vector that would cross
// the end of a row is read element by element. Needed: ld % 8 == 0 and 16-byte-aligned bases.
//
// dl4j_skinny_gemm_grouped: the same block on a grid (column blocks, X, S) for the experts of a mixture-of-experts
// step of Ntok <= 64 tokens, expert e's matrix being rows [e K, (e + 1) K) of the stacked N-contiguous parameter. It
// reads cnt[e] / off[e] of the routing plan (csrc/moe.hip) on the device as dl4j_wq_gemm_grouped does: an idle
// expert's blocks leave before their first weight load, the others multiply the first ceil(cnt[e] / 16) fragments,
// the panel rows are gathered through src_of or read from the expert-sorted buffer, only live rows are written, and
// split-K partials are kept compactly, [S][Ntok * k][Np].
//
// The epilogue, the split-K partial layout and merge launches, the routing-plan prelude of the grouped product, the
// split rule and the operand checks are csrc/skinny_body.h's, shared with csrc/gemm_wq.hip.
#include "skinny_body.h"

namespace {

template <int LAY> struct SkLay;
template <> struct SkLay<0> {
  static constexpr int CW = 16, KC = 256, NFR = 1, NL = 2, NV = 8;     // NL loads of NV elements per lane and chunk
  typedef sk_u4 vec;
};
template <> struct SkLay<1> {
  static constexpr int CW = 128, KC = 128, NFR = 8, NL = 8, NV = 8;
  typedef sk_u4 vec;
};
template <> struct SkLay<2> {
  static constexpr int CW = 64, KC = 128, NFR = 4, NL = 8, NV = 4;
  typedef sk_u2 vec;
};

constexpr int sk_max(int a, int b) { return a > b ? a : b; }
// LDS of a block: the x panel, then reused for one wave's accumulators
template <int LAY, int MF> constexpr int sk_lds_bytes() {
  return sk_max(MF * 16 * (SkLay<LAY>::KC + 8) * 2, SkLay<LAY>::NFR * MF * 64 * 16);
}

// NV 16-bit elements at p, the first `live` of them from memory and zeros behind
template <typename V, int NV> __device__ __forceinline__ V sk_ld_part(const unsigned short* p, int live) {
  unsigned short t[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) t[e] = e < live ? p[e] : (unsigned short)0;
  V v;
  __builtin_memcpy(&v, t, sizeof(V));
  return v;
}

// the lane's weight registers of the chunk quarter that starts at k = kw
template <typename hb, int LAY>
__device__ __forceinline__ void sk_load(const hb* __restrict__ W, long long ldw, int N, int K, int n0, int kw, int q,
                                        int c, typename SkLay<LAY>::vec (&w)[SkLay<LAY>::NL]) {
  using L = SkLay<LAY>;
  using V = typename L::vec;
  if constexpr (LAY == 0) {
    const int n = n0 + c;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = kw + 32 * j + 8 * q;
      w[j] = V{0u, 0u, 0u, 0u};
      if (n < N && k < K) {
        const hb* p = W + (long long)n * ldw + k;
        if (k + 8 <= K) w[j] = *reinterpret_cast<const V*>(p);
        else w[j] = sk_ld_part<V, 8>(reinterpret_cast<const unsigned short*>(p), K - k);
      }
    }
  } else {
    const int n = n0 + L::NV * c;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = kw + 8 * q + i;
      V v;
      __builtin_memset(&v, 0, sizeof(V));
      if (n < N && k < K) {
        const hb* p = W + (long long)k * ldw + n;
        if (n + L::NV <= N) v = *reinterpret_cast<const V*>(p);
        else v = sk_ld_part<V, L::NV>(reinterpret_cast<const unsigned short*>(p), N - n);
      }
      w[i] = v;
    }
  }
}

// The K loop of one block and the waves' sum: on return wave 3 holds, in acc[t][f][r], the block's sum for token
// 16 f + c and column n0 + NC q + NFR r + t (NC = 4 NFR consecutive columns per lane). src(r): the x row of panel row
// r or -1 for zeros; mfl: the live fragments (block-uniform).
template <typename hb, int MF, int LAY, typename Src>
__device__ __forceinline__ void sk_block(const hb* __restrict__ W, long long ldw, const hb* __restrict__ x, int ldx,
                                         Src src, int mfl, int N, int K, int n0, int ch0, int ch1,
                                         unsigned char* smem, sk_f4 (&acc)[SkLay<LAY>::NFR][MF]) {
  using L = SkLay<LAY>;
  using V = typename L::vec;
  constexpr int KC = L::KC, KW = KC / 4, LDX = KC + 8, NFR = L::NFR;
  hb* xs = reinterpret_cast<hb*>(smem);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
#pragma unroll
  for (int t = 0; t < NFR; ++t)
#pragma unroll
    for (int f = 0; f < MF; ++f) acc[t][f] = sk_f4{0.f, 0.f, 0.f, 0.f};

  V w[L::NL], wn[L::NL];
  if (ch0 < ch1) sk_load<hb, LAY>(W, ldw, N, K, n0, ch0 * KC + wave * KW, q, c, w);
  for (int ch = ch0; ch < ch1; ++ch) {
    __syncthreads();                                                   // the previous chunk's fragment reads are done
    const int kc = ch * KC;
    for (int i = tid; i < mfl * 16 * (KC / 8); i += 256) {
      const int r = i / (KC / 8), k8 = (i % (KC / 8)) * 8;
      const int sr = src(r);
      sk_u4 v = sk_u4{0u, 0u, 0u, 0u};
      if (sr >= 0 && kc + k8 < K) {
        const hb* p = x + (long long)sr * ldx + kc + k8;
        if (kc + k8 + 8 <= K) v = *reinterpret_cast<const sk_u4*>(p);
        else v = sk_ld_part<sk_u4, 8>(reinterpret_cast<const unsigned short*>(p), K - kc - k8);
      }
      *reinterpret_cast<sk_u4*>(xs + r * LDX + k8) = v;
    }
    if (ch + 1 < ch1) sk_load<hb, LAY>(W, ldw, N, K, n0, kc + KC + wave * KW, q, c, wn);   // in flight over the MFMAs
    __syncthreads();
    if (kc + wave * KW < K) {                                          // wave-uniform
      if constexpr (LAY == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const SV8<hb> a = __builtin_bit_cast(SV8<hb>, w[j]);
#pragma unroll
          for (int f = 0; f < MF; ++f)
            if (f < mfl) {
              const SV8<hb> b = *reinterpret_cast<const SV8<hb>*>(xs + (f * 16 + c) * LDX + wave * KW + 32 * j + 8 * q);
              acc[0][f] = sk_mma(a, b, acc[0][f]);
            }
        }
      } else {
        SV8<hb> b[MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) {
          b[f] = SV8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
          if (f < mfl) b[f] = *reinterpret_cast<const SV8<hb>*>(xs + (f * 16 + c) * LDX + wave * KW + 8 * q);
        }
#pragma unroll
        for (int t = 0; t < NFR; ++t) {
          // element t of the 8 row vectors: dword t / 2 of each, its low or high half
          const unsigned sel = (t & 1) ? 0x07060302u : 0x05040100u;
          sk_u4 av;
#pragma unroll
          for (int p = 0; p < 4; ++p) av[p] = __builtin_amdgcn_perm(w[2 * p + 1][t >> 1], w[2 * p][t >> 1], sel);
          const SV8<hb> a = __builtin_bit_cast(SV8<hb>, av);
#pragma unroll
          for (int f = 0; f < MF; ++f)
            if (f < mfl) acc[t][f] = sk_mma(a, b[f], acc[t][f]);       // block-uniform: dead fragments cost nothing
        }
      }
    }
    if (ch + 1 < ch1) {
#pragma unroll
      for (int i = 0; i < L::NL; ++i) w[i] = wn[i];
    }
  }
  // the four waves' sums in wave order: ((w0 + w1) + w2) + w3, one wave's accumulators in LDS at a time
  sk_f4* red = reinterpret_cast<sk_f4*>(smem);
  __syncthreads();
#pragma unroll
  for (int wv = 0; wv < 3; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int t = 0; t < NFR; ++t)
#pragma unroll
        for (int f = 0; f < MF; ++f)
          if (f < mfl) {
            sk_f4* slot = red + (t * MF + f) * 64 + lane;
            *slot = wv == 0 ? acc[t][f] : *slot + acc[t][f];
          }
    }
    __syncthreads();
  }
  if (wave == 3) {
#pragma unroll
    for (int t = 0; t < NFR; ++t)
#pragma unroll
      for (int f = 0; f < MF; ++f)
        if (f < mfl) acc[t][f] = red[(t * MF + f) * 64 + lane] + acc[t][f];
  }
}

// wave 3's accumulators of fragment f as the lane's NC consecutive columns
template <int LAY, int MF>
__device__ __forceinline__ void sk_lane_row(const sk_f4 (&acc)[SkLay<LAY>::NFR][MF], int f, float* vals) {
  constexpr int NFR = SkLay<LAY>::NFR;
#pragma unroll
  for (int t = 0; t < NFR; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) vals[r * NFR + t] = acc[t][f][r];
}

template <int NC> __device__ __forceinline__ void sk_store_partial(float* p, const float* vals) {
#pragma unroll
  for (int g = 0; g < NC / 4; ++g)
    *reinterpret_cast<sk_f4*>(p + 4 * g) = sk_f4{vals[4 * g], vals[4 * g + 1], vals[4 * g + 2], vals[4 * g + 3]};
}

template <typename hb, int NC>
__device__ __forceinline__ void sk_finish(const SkEpi& e, const float* vals, int m, int n, int N) {
  constexpr int G = NC >= 8 ? 8 : 4;
#pragma unroll
  for (int g = 0; g < NC / G; ++g) sk_epilogue<hb, G>(e, vals + g * G, m, n + g * G, N);
}

template <typename hb, int MF, int LAY>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(const hb* __restrict__ W, long long ldw,
                                                          const hb* __restrict__ x, int ldx, int M, int N, int K,
                                                          int cpb, float* __restrict__ ws, SkEpi epi) {
  using L = SkLay<LAY>;
  constexpr int NC = 4 * L::NFR;
  __shared__ __attribute__((aligned(16))) unsigned char smem[sk_lds_bytes<LAY, MF>()];
  const int NCH = (K + L::KC - 1) / L::KC;
  const int ch0 = blockIdx.y * cpb, ch1 = min(NCH, ch0 + cpb);
  const int n0 = blockIdx.x * L::CW;
  sk_f4 acc[L::NFR][MF];
  sk_block<hb, MF, LAY>(W, ldw, x, ldx, [M](int r) { return r < M ? r : -1; }, MF, N, K, n0, ch0, ch1, smem, acc);
  if ((threadIdx.x >> 6) != 3) return;
  const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const int Np = gridDim.x * L::CW, n = n0 + NC * q;
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int m = f * 16 + c;
    if (m >= M) continue;
    float vals[NC];
    sk_lane_row<LAY, MF>(acc, f, vals);
    if (gridDim.y > 1) sk_store_partial<NC>(sk_partial(ws, blockIdx.y, M, m, Np, n), vals);
    else sk_finish<hb, NC>(epi, vals, m, n, N);
  }
}

// Block (nb, e, s) of the grouped product: skinny_gemm_kernel's body on expert e's rows of the stacked parameter, over
// the expert's live rows only.
template <typename hb, int MF, int LAY, bool GATHER>
__global__ __launch_bounds__(256) void skinny_grouped_kernel(const hb* __restrict__ W, long long ldw,
                                                             const hb* __restrict__ x, int ldx, SkPlan p, int N, int K,
                                                             int cpb, float* __restrict__ ws, SkEpi epi) {
  using L = SkLay<LAY>;
  constexpr int NC = 4 * L::NFR;
  __shared__ __attribute__((aligned(16))) unsigned char smem[sk_lds_bytes<LAY, MF>()];
  __shared__ int rowsrc[MF * 16];                                          // the x row of panel row r, -1: zeros
  const int tid = threadIdx.x;
  const int e = blockIdx.y;
  const SkGroup g = sk_group<MF>(p, e);
  if (g.rows <= 0) return;                                                 // block-uniform: no byte of an idle expert
  sk_group_rows<MF, GATHER>(p, g, rowsrc);
  const int NCH = (K + L::KC - 1) / L::KC;
  const int ch0 = blockIdx.z * cpb, ch1 = min(NCH, ch0 + cpb);
  const int n0 = blockIdx.x * L::CW;
  sk_f4 acc[L::NFR][MF];
  // rowsrc is read behind the body's first barrier
  sk_block<hb, MF, LAY>(W + (long long)e * K * ldw, ldw, x, ldx, [&](int r) { return rowsrc[r]; }, g.mfl, N, K, n0,
                        ch0, ch1, smem, acc);
  if ((tid >> 6) != 3) return;
  const int lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int Np = gridDim.x * L::CW, n = n0 + NC * q;
  const int pre = gridDim.z > 1 ? sk_group_pre(p, e) : 0;
  const SkEpi le = sk_expert_epi(epi, e, N);
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int m = f * 16 + c;
    if (f >= g.mfl || m >= g.rows) continue;
    float vals[NC];
    sk_lane_row<LAY, MF>(acc, f, vals);
    if (gridDim.z > 1) {
      const int cr = pre + m;                                              // the compact row
      if (cr >= 0 && cr < p.A) sk_store_partial<NC>(sk_partial(ws, blockIdx.z, p.A, cr, Np, n), vals);
    } else {
      sk_finish<hb, NC>(le, vals, g.off + m, n, N);
    }
  }
}

inline int sk_cw(int lay) { return lay == 0 ? 16 : (lay == 1 ? 128 : 64); }
inline int sk_kc(int lay) { return lay == 0 ? 256 : 128; }
inline bool sk_shape_ok(long long K, long long N) { return K >= 1 && N >= 1 && K <= (1 << 24) && N <= (1 << 24); }

// Load width of the N-contiguous layout from (M, N, K) alone: the 8-byte loads' 64-column blocks while 128-column
// blocks with every K chunk on a block of its own would leave compute units idle; 16-byte loads beyond. Measured
// (profiles/skinny_gemm.txt): at the decode shapes up to (768, 3072) the 8-byte loads are 0.7 to 3.8 us faster at
// every M; shapes beyond the threshold are not measured.
inline int sk_width_rule(int M, long long N, long long K) {
  (void)M;
  const long long blocks = ((N + 127) / 128) * ((K + 127) / 128);
  return blocks < 256 ? 4 : 8;
}

// the layout: 0 for K-contiguous weights, 1 / 2 for N-contiguous ones read 8 / 4 columns per lane (width 8 / 4, 0: the
// rule); -1: strides the kernels do not take
inline int sk_layout(int width, int M, long long N, long long K, long long sk, long long sn) {
  if (width != 0 && width != 4 && width != 8) return -1;
  if (sn == 1 && sk >= N && sk % 8 == 0) {
    const int wd = width ? width : sk_width_rule(M, N, K);
    return wd == 8 ? 1 : 2;
  }
  if (sk == 1 && sn >= K && sn % 8 == 0) return 0;
  return -1;
}

// split count and chunks per block from (layout, M, N, K) alone: sk_split_plan on the layout's column blocks and chunk
// depth, 16 weight bits per element
inline void sk_split(int lay, int M, long long N, long long K, int* S, int* cpb) {
  sk_split_plan(sk_cw(lay), sk_kc(lay), 16, M, N, K, S, cpb);
}
// sk_split for the grouped product, from (layout, Ntok, k, X, N, K) alone
inline void sk_split_grouped(int lay, int Ntok, int k, int X, long long N, long long K, int* S, int* cpb) {
  sk_split_plan_grouped(sk_cw(lay), sk_kc(lay), 16, Ntok, k, X, N, K, S, cpb);
}

inline bool sk_grouped_ok(int width, int Ntok, int k, int X, long long N, long long K) {
  return (width == 0 || width == 4 || width == 8) && sk_shape_ok(K, N) && sk_routing_ok(Ntok, k, X) &&
         (long long)X * K <= (1LL << 31);
}

inline int sk_grouped_layout(int width, int Ntok, int k, int X, long long N, long long K) {
  const int A = Ntok * k;
  const int wd = width ? width : sk_width_rule(Ntok, N * (X < A ? X : A), K);
  return wd == 8 ? 1 : 2;
}

}  // namespace

// Floats of split-K workspace dl4j_skinny_gemm needs for W [K, N] with element strides (sk, sn): 0 when the product
// runs unsplit, -1 for operands it refuses. width: the load width of the N-contiguous layout, 8 / 4 columns per lane,
// 0 for the rule on (M, N, K).
DL4J_API long long dl4j_skinny_gemm_workspace(int width, int M, long long N, long long K, long long sk, long long sn) {
  if (!sk_shape_ok(K, N) || M < 1 || M > 64) return -1;
  const int lay = sk_layout(width, M, N, K, sk, sn);
  if (lay < 0) return -1;
  int S, cpb;
  sk_split(lay, M, N, K, &S, &cpb);
  return sk_ws_floats(S, M, N, sk_cw(lay));
}

// out [M, ldo] = act(x [M, ldx] · W + bias + beta·out), 1 <= M <= 64, W [K, N] of the same dtype read in place with
// element strides (sk, sn): N-contiguous (sn 1, sk % 8 == 0) or K-contiguous (sk 1, sn % 8 == 0), base 16-byte
// aligned. dtype 1 bf16 / 2 fp16 (x, W and out); bias [N] of dtype bias_dt (0 fp32, 1, 2) or null; beta 0 / 1; act 0
// none / 4 GELU; ws: the floats dl4j_skinny_gemm_workspace asks for (may be null when 0). -1: refused (shape, strides,
// alignment, dtype), nothing launched.
DL4J_API int dl4j_skinny_gemm(int width, int dtype, const void* x, long long ldx, int M, long long N, long long K,
                              const void* W, long long sk, long long sn, void* out, long long ldo, const void* bias,
                              int bias_dt, int beta, int act, void* ws, hipStream_t s) {
  if (!sk_shape_ok(K, N) || !sk_dense_ok(M, beta, bias_dt) || !sk_operands_ok(dtype, x, ldx, K, out, ldo, N, act))
    return -1;
  const int lay = sk_layout(width, M, N, K, sk, sn);
  if (lay < 0 || !sk_al16(W)) return -1;
  int S, cpb;
  sk_split(lay, M, N, K, &S, &cpb);
  if (S > 1 && !sk_al16(ws)) return -1;
  const int cw = sk_cw(lay), nbk = (int)((N + cw - 1) / cw);
  const long long ldw = lay == 0 ? sn : sk;
  const SkEpi epi{out, bias, (int)ldo, bias_dt, beta, act};
  const dim3 grid((unsigned)nbk, (unsigned)S);
  const int mf = sk_mf(M);
#define L(T, F, Y) hipLaunchKernelGGL((skinny_gemm_kernel<T, F, Y>), grid, dim3(256), 0, s, (const T*)W, ldw,        \
                                      (const T*)x, (int)ldx, M, (int)N, (int)K, cpb, (float*)ws, epi)
#define LY(T, F) do { if (lay == 0) L(T, F, 0); else if (lay == 1) L(T, F, 1); else L(T, F, 2); } while (0)
#define LM(T) do { if (mf == 1) LY(T, 1); else if (mf == 2) LY(T, 2); else LY(T, 4); } while (0)
  if (dtype == 1) LM(__bf16);
  else LM(_Float16);
#undef LM
#undef LY
#undef L
  const int rc = (int)hipGetLastError();
  return rc != 0 || S == 1 ? rc : sk_merge(dtype, ws, S, M, (int)N, nbk * cw, epi, s);
}

// Floats of split-K workspace dl4j_skinny_gemm_grouped needs for (width, Ntok, k, X, N, K): 0 when the product runs
// unsplit, -1 for a shape it refuses.
DL4J_API long long dl4j_skinny_gemm_grouped_workspace(int width, int Ntok, int k, int X, long long N, long long K) {
  if (!sk_grouped_ok(width, Ntok, k, X, N, K)) return -1;
  const int lay = sk_grouped_layout(width, Ntok, k, X, N, K);
  int S, cpb;
  sk_split_grouped(lay, Ntok, k, X, N, K, &S, &cpb);
  return sk_ws_floats(S, (long long)Ntok * k, N, sk_cw(lay));
}

// The experts' products of a mixture-of-experts step of Ntok <= 64 tokens on the stacked N-contiguous parameter W
// [X * K, N] (row pitch ldw, ldw % 8 == 0, 16-byte aligned; expert e's matrix is rows [e K, (e + 1) K)), read in
// place: out[off[e] + r] = act(row_r · W_e + bias[e]) for r < cnt[e], with cnt [X], off [X + 1] and src_of [Rcap] the
// plan of dl4j_moe_route for (Ntok, k, X). gather 1: row_r = x[src_of[off[e] + r] / k], x the token-major activations
// [Ntok, ldx]; gather 0: row_r = x[off[e] + r], x an expert-sorted buffer [Rcap, ldx] (src_of may be null). out [Rcap,
// ldo]: pad rows and the segments of idle experts are not written. dtype 1 bf16 / 2 fp16; bias fp32 [X, N] or null;
// act 0 none / 4 GELU; ws: the floats dl4j_skinny_gemm_grouped_workspace asks for (may be null when 0). The plan is
// read on the device only. -1: refused (shape, Ntok > 64, alignment, dtype), nothing launched.
DL4J_API int dl4j_skinny_gemm_grouped(int width, int dtype, const void* x, long long ldx, int gather, int Ntok, int k,
                                      int X, long long Rcap, long long N, long long K, const void* W, long long ldw,
                                      const int* cnt, const int* off, const int* src_of, void* out, long long ldo,
                                      const float* bias, int act, void* ws, hipStream_t s) {
  if (!sk_grouped_ok(width, Ntok, k, X, N, K) || !sk_operands_ok(dtype, x, ldx, K, out, ldo, N, act)) return -1;
  if (!sk_plan_ok(gather, Ntok, k, Rcap, cnt, off, src_of, bias) || !sk_al16(W) || ldw % 8 != 0 || ldw < N) return -1;
  const int lay = sk_grouped_layout(width, Ntok, k, X, N, K);
  int S, cpb;
  sk_split_grouped(lay, Ntok, k, X, N, K, &S, &cpb);
  if (S > 1 && !sk_al16(ws)) return -1;
  const int cw = sk_cw(lay), nbk = (int)((N + cw - 1) / cw);
  const SkEpi epi{out, bias, (int)ldo, 0, 0, act};
  const SkPlan plan{cnt, off, src_of, Ntok, k, X, Ntok * k, Rcap};
  const dim3 grid((unsigned)nbk, (unsigned)X, (unsigned)S);
  const int mf = sk_mf(Ntok);
#define L(T, F, Y, G) hipLaunchKernelGGL((skinny_grouped_kernel<T, F, Y, G>), grid, dim3(256), 0, s, (const T*)W,    \
                                         ldw, (const T*)x, (int)ldx, plan, (int)N, (int)K, cpb, (float*)ws, epi)
#define LG(T, F, Y) do { if (gather) L(T, F, Y, true); else L(T, F, Y, false); } while (0)
#define LY(T, F) do { if (lay == 1) LG(T, F, 1); else LG(T, F, 2); } while (0)
#define LM(T) do { if (mf == 1) LY(T, 1); else if (mf == 2) LY(T, 2); else LY(T, 4); } while (0)
  if (dtype == 1) LM(__bf16);
  else LM(_Float16);
#undef LM
#undef LY
#undef LG
#undef L
  const int rc = (int)hipGetLastError();
  return rc != 0 || S == 1 ? rc : sk_merge_grouped(dtype, ws, S, plan, (int)N, nbk * cw, epi, s);
}
