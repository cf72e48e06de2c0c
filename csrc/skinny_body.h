// What the decode-time skinny products (M <= 64 rows) share: the 16-bit product on the weights in place
// (csrc/gemm_skinny.hip) and the weight-only MXFP8 / MXFP4 product (csrc/gemm_wq.hip), each dense and grouped per
// expert of a mixture-of-experts step. The K loops stay in those files (one prefetches three register layouts across
// the MFMAs, the other loads a packed tile per chunk); a change to the epilogue, the routing-plan contract, the
// split-K partial layout or the split rule is made here, once. Both files include this header and instantiate what
// they use in their own translation unit.
//
//  * epilogue: per element acc + bias + beta·out in fp32, GELU, ONE rounding to the 16-bit output (sk_epilogue).
//  * split-K: when the column blocks alone do not cover the chip the grid splits K; split s of row r writes its fp32
//    sums to plane s of a workspace [S][R][Np] (sk_partial; R = M rows, or the Ntok * k compact rows of a grouped
//    product, Np = N padded to the column block) and a merge launch sums the planes in split order and applies the
//    epilogue. No float atomics anywhere: two runs give the same bits.
//  * grouped products read cnt[e] / off[e] / src_of of the routing plan (csrc/moe.hip) on the device: sk_group holds
//    an expert's rows to what the block and the sorted buffer can take, sk_group_rows says which x row each panel row
//    reads. An idle expert's blocks must leave on rows <= 0 before their first weight load.
//  * the split rule (sk_split_plan / sk_split_plan_grouped) and the refusal checks of the entry points.
#pragma once
#include "common.h"
#include "mfma_tile.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float sk_f4;
typedef __attribute__((ext_vector_type(4))) unsigned sk_u4;
typedef __attribute__((ext_vector_type(2))) unsigned sk_u2;
template <typename T> using SV8 = T __attribute__((ext_vector_type(8)));
template <typename T> using SV4 = T __attribute__((ext_vector_type(4)));

__device__ __forceinline__ sk_f4 sk_mma(SV8<__bf16> a, SV8<__bf16> b, sk_f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ sk_f4 sk_mma(SV8<_Float16> a, SV8<_Float16> b, sk_f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

struct SkEpi {
  void* out;             // [M, ldo] 16-bit
  const void* bias;      // [N] or null
  int ldo, bias_dt, beta, act;
};

// G consecutive columns n .. n + G - 1 of row m (G 4 / 8): bias, beta·out, activation, one rounding; one vector store
// where the G columns exist and out + n is aligned to it, masked element stores elsewhere
template <typename hb, int G>
__device__ __forceinline__ void sk_epilogue(const SkEpi& e, const float* v, int m, int n, int N) {
  if (n >= N) return;
  hb* o = reinterpret_cast<hb*>(e.out) + (long long)m * e.ldo + n;
  typedef hb OV __attribute__((ext_vector_type(G)));
  const bool whole = n + G <= N && (reinterpret_cast<uintptr_t>(o) & (2 * G - 1)) == 0;
  float t[G];
#pragma unroll
  for (int r = 0; r < G; ++r) t[r] = v[r];
  if (e.bias) {
#pragma unroll
    for (int r = 0; r < G; ++r)
      if (n + r < N) t[r] += ld_any(e.bias, e.bias_dt, n + r);
  }
  if (e.beta) {
    if (whole) {
      const OV old = *reinterpret_cast<const OV*>(o);
#pragma unroll
      for (int r = 0; r < G; ++r) t[r] += (float)old[r];
    } else {
#pragma unroll
      for (int r = 0; r < G; ++r)
        if (n + r < N) t[r] += (float)o[r];
    }
  }
  if (e.act == 4) {
#pragma unroll
    for (int r = 0; r < G; ++r) t[r] = gelu_f(t[r]);
  }
  if (whole) {
    OV nv;
#pragma unroll
    for (int r = 0; r < G; ++r) nv[r] = (hb)t[r];
    *reinterpret_cast<OV*>(o) = nv;
  } else {
#pragma unroll
    for (int r = 0; r < G; ++r)
      if (n + r < N) o[r] = (hb)t[r];
  }
}
template <typename hb> __device__ __forceinline__ void sk_epilogue4(const SkEpi& e, sk_f4 s, int m, int n, int N) {
  const float vals[4] = {s[0], s[1], s[2], s[3]};
  sk_epilogue<hb, 4>(e, vals, m, n, N);
}

// column n of row `row` in plane `split` of the split-K workspace [S][R][Np]
__device__ __forceinline__ float* sk_partial(float* ws, int split, int R, int row, int Np, int n) {
  return ws + ((long long)split * R + row) * Np + n;
}
// the S planes' four columns from n of a row, summed in split order
__device__ __forceinline__ sk_f4 sk_merge_sum(const float* ws, int S, int R, int row, int Np, int n) {
  sk_f4 s = *reinterpret_cast<const sk_f4*>(ws + (long long)row * Np + n);
  for (int p = 1; p < S; ++p) s += *reinterpret_cast<const sk_f4*>(ws + ((long long)p * R + row) * Np + n);
  return s;
}

// split-K merge: the S partial planes [M, Np] summed in split order, then the epilogue
template <typename hb>
__global__ __launch_bounds__(256) void skinny_merge_kernel(const float* __restrict__ ws, int S, int M, int N, int Np,
                                                           SkEpi epi) {
  const int q4 = Np >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * q4) return;
  const int m = idx / q4, n = (idx - m * q4) * 4;
  if (n >= N) return;
  sk_epilogue4<hb>(epi, sk_merge_sum(ws, S, M, m, Np, n), m, n, N);
}

// The routing plan of csrc/moe.hip as the grouped products read it (device pointers, int32).
struct SkPlan {
  const int* cnt;      // [X] assignments per expert
  const int* off;      // [X + 1] first row of every expert's segment of the sorted buffers
  const int* src_of;   // [Rcap] assignment n*k + j of a live row; read in gather mode only
  int Ntok, k, X, A;   // A = Ntok * k
  long long Rcap;
};

// Expert e's share of a grouped product in a block of MF fragments: rows = cnt[e], held to the MF fragments and to the
// sorted buffer whatever the plan holds, and mfl live fragments. rows <= 0 is an idle expert (block-uniform): its
// blocks must return on it before any weight load.
struct SkGroup {
  int off, rows, mfl;
};
template <int MF> __device__ __forceinline__ SkGroup sk_group(const SkPlan& p, int e) {
  const int off = p.off[e];
  const long long room = p.Rcap - off;
  const int rows = off < 0 ? 0 : (int)min((long long)min(p.cnt[e], MF * 16), room);
  return SkGroup{off, rows, (rows + 15) >> 4};
}
// rowsrc[r], the x row of panel row r < 16 MF (-1: zeros): the token of the plan's assignment in gather mode, row
// off + r of the expert-sorted buffer else. Readable behind the next barrier.
template <int MF, bool GATHER>
__device__ __forceinline__ void sk_group_rows(const SkPlan& p, const SkGroup& g, int* rowsrc) {
  const int tid = threadIdx.x;
  if (tid < MF * 16) {
    int src = -1;
    if (tid < g.rows) {
      if (GATHER) {
        const int a = p.src_of[g.off + tid];
        src = (a >= 0 && a < p.A) ? a / p.k : -1;
      } else {
        src = g.off + tid;
      }
    }
    rowsrc[tid] = src;
  }
}
// the compact row of expert e's first live row in the split-K partials: the exclusive prefix of cnt
__device__ __forceinline__ int sk_group_pre(const SkPlan& p, int e) {
  int pre = 0;
  for (int i = 0; i < e; ++i) pre += p.cnt[i];
  return pre;
}
// the epilogue of expert e: its row of the fp32 bias [X, N]
__device__ __forceinline__ SkEpi sk_expert_epi(const SkEpi& epi, int e, int N) {
  SkEpi le = epi;
  if (epi.bias) le.bias = reinterpret_cast<const float*>(epi.bias) + (long long)e * N;
  return le;
}

// split-K merge of a grouped product: compact row cr belongs to the expert e whose prefix of cnt covers it; the S
// partial planes [A, Np] summed in split order, then the epilogue into row off[e] + r
template <typename hb>
__global__ __launch_bounds__(256) void skinny_merge_grouped_kernel(const float* __restrict__ ws, int S, SkPlan p,
                                                                   int mrows, int N, int Np, SkEpi epi) {
  const int q4 = Np >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.A * q4) return;
  const int cr = idx / q4, n = (idx - cr * q4) * 4;
  if (n >= N) return;
  int e = 0, run = 0;
  for (; e < p.X; ++e) {
    const int ce = p.cnt[e];
    if (cr < run + ce) break;
    run += ce;
  }
  if (e >= p.X) return;
  const int r = cr - run, off = p.off[e];
  if (r < 0 || r >= mrows || off < 0 || (long long)off + r >= p.Rcap) return;     // what the product's blocks wrote
  sk_epilogue4<hb>(sk_expert_epi(epi, e, N), sk_merge_sum(ws, S, p.A, cr, Np, n), off + r, n, N);
}

// ------------------------------------------------------------------------------------------------------------ host
inline bool sk_al16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool sk_al4(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline int sk_mf(int M) { return M <= 16 ? 1 : (M <= 32 ? 2 : 4); }              // column fragments of M rows

// Split count and chunks per block of a dense product from (column-block width cw, chunk depth kc, weight bits per
// element, M, N, K) alone: enough blocks for two per compute unit, but never so many that the fp32 partials (written
// and read once: 8 S M Np bytes) outweigh the weight bytes (K Np bits / 8)
inline void sk_split_plan(int cw, int kc, int bits, int M, long long N, long long K, int* S, int* cpb) {
  const long long nbk = (N + cw - 1) / cw;
  const int NCH = (int)((K + kc - 1) / kc);
  long long s = (512 + nbk - 1) / nbk;
  const long long cap = K * bits / (64LL * M);
  if (s > cap) s = cap;
  if (s > NCH) s = NCH;
  if (s < 1) s = 1;
  *cpb = (NCH + (int)s - 1) / (int)s;
  *S = (NCH + *cpb - 1) / *cpb;
}
// sk_split_plan for a grouped product, from (cw, kc, bits, Ntok, k, X, N, K) alone: min(X, Ntok * k) experts count as
// active (the blocks of the others leave at once), and the partials of the Ntok * k live rows are weighed against
// those experts' weight bytes
inline void sk_split_plan_grouped(int cw, int kc, int bits, int Ntok, int k, int X, long long N, long long K, int* S,
                                  int* cpb) {
  const long long nbk = (N + cw - 1) / cw;
  const int NCH = (int)((K + kc - 1) / kc);
  const int A = Ntok * k, active = X < A ? X : A;
  const long long blocks = nbk * active;
  long long s = (512 + blocks - 1) / blocks;
  const long long cap = (long long)active * K * bits / (64LL * A);
  if (s > cap) s = cap;
  if (s > NCH) s = NCH;
  if (s < 1) s = 1;
  *cpb = (NCH + (int)s - 1) / (int)s;
  *S = (NCH + *cpb - 1) / *cpb;
}

inline int sk_padded(long long N, int cw) { return (int)((N + cw - 1) / cw) * cw; }
// floats of split-K workspace for S planes of `rows` rows: none for an unsplit product
inline long long sk_ws_floats(int S, long long rows, long long N, int cw) {
  return S > 1 ? S * rows * sk_padded(N, cw) : 0;
}

// what the four entry points ask of x, out and the activation alike
inline bool sk_operands_ok(int dtype, const void* x, long long ldx, long long K, const void* out, long long ldo,
                           long long N, int act) {
  return (dtype == 1 || dtype == 2) && sk_al16(x) && ldx % 8 == 0 && ldx >= K && ldx <= 0x7fffffffLL && out &&
         ldo >= N && ldo <= 0x7fffffffLL && (act == 0 || act == 4);
}
// ... the dense ones of rows and epilogue
inline bool sk_dense_ok(int M, int beta, int bias_dt) {
  return M >= 1 && M <= 64 && (beta == 0 || beta == 1) && bias_dt >= 0 && bias_dt <= 2;
}
// ... the grouped ones of the plan's sizes (also what their workspace queries take) and of its operands
inline bool sk_routing_ok(int Ntok, int k, int X) {
  return Ntok >= 1 && Ntok <= 64 && k >= 1 && k <= 8 && X >= 1 && X <= 64 && k <= X;
}
inline bool sk_plan_ok(int gather, int Ntok, int k, long long Rcap, const int* cnt, const int* off, const int* src_of,
                       const float* bias) {
  return (gather == 0 || gather == 1) && Rcap >= (long long)Ntok * k && Rcap <= 0x7fffffffLL && sk_al4(cnt) &&
         sk_al4(off) && (!gather || sk_al4(src_of)) && (!bias || sk_al4(bias));
}

// the merge launch behind a split product's blocks: one thread per four columns of every row
inline int sk_merge(int dtype, const void* ws, int S, int M, int N, int Np, const SkEpi& epi, hipStream_t s) {
  const dim3 mg((unsigned)(((long long)M * (Np / 4) + 255) / 256));
  if (dtype == 1)
    hipLaunchKernelGGL(skinny_merge_kernel<__bf16>, mg, dim3(256), 0, s, (const float*)ws, S, M, N, Np, epi);
  else
    hipLaunchKernelGGL(skinny_merge_kernel<_Float16>, mg, dim3(256), 0, s, (const float*)ws, S, M, N, Np, epi);
  return (int)hipGetLastError();
}
inline int sk_merge_grouped(int dtype, const void* ws, int S, const SkPlan& plan, int N, int Np, const SkEpi& epi,
                            hipStream_t s) {
  const dim3 mg((unsigned)(((long long)plan.A * (Np / 4) + 255) / 256));
  const int mrows = sk_mf(plan.Ntok) * 16;
  if (dtype == 1)
    hipLaunchKernelGGL(skinny_merge_grouped_kernel<__bf16>, mg, dim3(256), 0, s, (const float*)ws, S, plan, mrows, N,
                       Np, epi);
  else
    hipLaunchKernelGGL(skinny_merge_grouped_kernel<_Float16>, mg, dim3(256), 0, s, (const float*)ws, S, plan, mrows, N,
                       Np, epi);
  return (int)hipGetLastError();
}

}  // namespace
