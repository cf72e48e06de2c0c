// Mixture-of-experts feed-forward for gfx950: top-k router, the device-side plan that sorts the (token, choice)
// assignments by expert, and the permutation kernels around the grouped GEMM (csrc/gemm.hip, GRP modes).
//
// Routing contract (Mixtral's): for a token with fp32 logits l[0..X), the experts are ordered by (logit descending,
// index ascending); the first k are e_0 .. e_{k-1}, g_j = exp(l[e_j] - l[e_0]) / sum_{i<k} exp(l[e_i] - l[e_0]), stored in
// fp32. The k exponentials, their sum and the quotient are evaluated in fp64 and rounded once: the fp32 evaluation
// with the accurate expf is off by up to ~4.3 * 2^-24 relative for k = 8 (one ulp of expf, the rounding of l - l_0, the
// k - 1 additions and the division), which is past the 4 * 2^-24 the gates are held to. Selection compares the fp32
// logits themselves. Nothing is dropped.
//
// Plan (all int32, sized by shapes alone: A = N*k assignments, G = 128, Rcap = roundup(A + X*(G-1), G) rows):
//   idx[N,k], cnt[X], off[X+1] (off[e+1] = off[e] + roundup(cnt[e], G)), row_of[N,k] the row of assignment (n, j) in
//   the expert-sorted buffers, src_of[Rcap] = n*k + j for a live row and -1 for a pad row, tile_expert[Rcap/G] the
//   expert of a row tile or -1. Inside an expert's segment the rows are in (token, choice) order: a stable sort, so
//   the plan is a pure function of the logits. Counting uses integer LDS atomics only (exact, order-free); there are
//   no floating-point atomics anywhere and no count ever reaches the host.
//
//   dl4j_moe_route: moe_topk (one thread per token: selection, gates, a per-block histogram of 256 tokens, src_of
//   cleared) -> moe_scan (one block: counts, per-block bases, off, tile_expert) -> moe_scatter (rank of every
//   assignment among the earlier ones of its block with the same expert, by wave ballots -> row_of, src_of).
//
// Rows of dead tiles (tile_expert = -1) are never written by the gather and never read by anything.
#include "common.h"

namespace {

constexpr int kMoeTile = 128;      // G: the row tile of the grouped GEMM
constexpr int kMoeMaxX = 64;
constexpr int kMoeMaxK = 8;
constexpr int kMoeTok = 256;       // tokens per block of the routing kernels

__global__ __launch_bounds__(kMoeTok) void moe_topk_kernel(const float* __restrict__ logits, long long N, int X, int k,
                                                           int* __restrict__ idx, float* __restrict__ gate,
                                                           int* __restrict__ hist, int* __restrict__ src_of,
                                                           long long Rcap) {
  __shared__ int h[kMoeMaxX];
  if (threadIdx.x < kMoeMaxX) h[threadIdx.x] = 0;
  __syncthreads();
  for (long long r = (long long)blockIdx.x * kMoeTok + threadIdx.x; r < Rcap; r += (long long)gridDim.x * kMoeTok)
    src_of[r] = -1;
  const long long n = (long long)blockIdx.x * kMoeTok + threadIdx.x;
  if (n < N) {
    const float* l = logits + n * X;
    unsigned long long taken = 0ull;
    double v[kMoeMaxK];
    double sum = 0.0;
    float top = 0.f;
#pragma unroll
    for (int j = 0; j < kMoeMaxK; ++j) {
      v[j] = 0.0;
      if (j < k) {
        int best = -1;
        float bv = 0.f;
        for (int e = 0; e < X; ++e) {
          if ((taken >> e) & 1ull) continue;
          const float x = l[e];
          if (best < 0 || x > bv) {            // strict: among equal logits the lowest index wins
            best = e;
            bv = x;
          }
        }
        taken |= 1ull << best;
        if (j == 0) top = bv;
        v[j] = exp((double)bv - (double)top);
        sum += v[j];
        idx[n * k + j] = best;
        atomicAdd(&h[best], 1);
      }
    }
#pragma unroll
    for (int j = 0; j < kMoeMaxK; ++j)
      if (j < k) gate[n * k + j] = (float)(v[j] / sum);
  }
  __syncthreads();
  if (threadIdx.x < X) hist[(long long)blockIdx.x * X + threadIdx.x] = h[threadIdx.x];
}

// one block: hist[c][e] -> the number of assignments to e in the blocks before c; cnt, off, tile_expert
__global__ __launch_bounds__(256) void moe_scan_kernel(int* __restrict__ hist, int nblk, int X, int* __restrict__ cnt,
                                                       int* __restrict__ off, int* __restrict__ tile_expert,
                                                       int ntiles) {
  __shared__ int scnt[kMoeMaxX];
  __shared__ int soff[kMoeMaxX + 1];
  const int tid = threadIdx.x;
  if (tid < X) {
    int run = 0;
    for (int c = 0; c < nblk; ++c) {
      const int t = hist[(long long)c * X + tid];
      hist[(long long)c * X + tid] = run;
      run += t;
    }
    cnt[tid] = run;
    scnt[tid] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int e = 0; e < X; ++e) {
      soff[e] = o;
      o += (scnt[e] + kMoeTile - 1) / kMoeTile * kMoeTile;
    }
    soff[X] = o;
  }
  __syncthreads();
  if (tid <= X) off[tid] = soff[tid];
  for (int t = tid; t < ntiles; t += 256) {
    const int r = t * kMoeTile;
    int ex = -1;
    if (r < soff[X])
      for (int e = 0; e < X; ++e)
        if (r < soff[e + 1]) {
          ex = e;
          break;
        }
    tile_expert[t] = ex;
  }
}

// rank of assignment (n, j) among the earlier ones of its block with the same expert. A token's k experts are distinct,
// so that is the number of earlier TOKENS of the block that chose the expert: per expert one wave ballot of "this
// token chose it" gives the count among the lower lanes and the wave's total; the earlier waves' totals are added
// through LDS. Linear in X per wave, integer only, a pure function of idx.
__global__ __launch_bounds__(kMoeTok) void moe_scatter_kernel(const int* __restrict__ idx, const int* __restrict__ base,
                                                              const int* __restrict__ off, long long N, int X, int k,
                                                              int* __restrict__ row_of, int* __restrict__ src_of) {
  __shared__ int wcnt[kMoeTok / 64][kMoeMaxX];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long long n = (long long)blockIdx.x * kMoeTok + threadIdx.x;
  int e[kMoeMaxK], rank[kMoeMaxK];
#pragma unroll
  for (int j = 0; j < kMoeMaxK; ++j) {
    e[j] = (j < k && n < N) ? idx[n * k + j] : -1;
    rank[j] = 0;
  }
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int x = 0; x < X; ++x) {
    bool has = false;
#pragma unroll
    for (int j = 0; j < kMoeMaxK; ++j) has |= e[j] == x;
    const unsigned long long m = __ballot(has);
    if (lane == 0) wcnt[wid][x] = __popcll(m);
    const int r = __popcll(m & lower);
#pragma unroll
    for (int j = 0; j < kMoeMaxK; ++j)
      if (e[j] == x) rank[j] = r;
  }
  __syncthreads();
  if (n >= N) return;
#pragma unroll
  for (int j = 0; j < kMoeMaxK; ++j) {
    if (j < k) {
      const int ex = e[j];
      int r = rank[j];
      for (int w = 0; w < wid; ++w) r += wcnt[w][ex];
      const int row = off[ex] + base[(long long)blockIdx.x * X + ex] + r;
      row_of[n * k + j] = row;
      src_of[row] = (int)(n * k + j);
    }
  }
}

// Xp[r] = scale[src_of[r]] * x[src_of[r] / k] (fp32 product, one rounding), zeros for a pad row; one wave per row
template <typename T>
__global__ __launch_bounds__(256) void moe_gather_kernel(const T* __restrict__ x, const int* __restrict__ src_of,
                                                         const int* __restrict__ tile_expert,
                                                         const float* __restrict__ scale, T* __restrict__ xp,
                                                         long long Rcap, int E8, int k) {
  const int lane = threadIdx.x & 63;
  const long long E = (long long)E8 * 8;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < Rcap; r += (long long)gridDim.x * 4) {
    if (tile_expert[r / kMoeTile] < 0) continue;
    const int src = src_of[r];
    const float sc = (src >= 0 && scale) ? scale[src] : 1.f;
    const T* in = x + (long long)(src < 0 ? 0 : src / k) * E;
    for (int c = lane; c < E8; c += 64) {
      float v[8];
      if (src >= 0) {
        Vec8<T>::load(in + c * 8, v);
        if (scale) {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] *= sc;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
      }
      Vec8<T>::store(xp + r * E + c * 8, v);
    }
  }
}

// y[n] = round(acc[n] + sum_j w[n,j] * Yp[row_of[n,j]]) in fp32, j ascending; one wave per token. acc may be y.
template <typename T>
__global__ __launch_bounds__(256) void moe_combine_kernel(const T* __restrict__ yp, const int* __restrict__ row_of,
                                                          const float* __restrict__ w, const T* acc, T* y,
                                                          long long N, int E8, int k) {
  const int lane = threadIdx.x & 63;
  const long long E = (long long)E8 * 8;
  for (long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); n < N; n += (long long)gridDim.x * 4) {
    for (int c = lane; c < E8; c += 64) {
      float s[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] = 0.f;
      for (int j = 0; j < k; ++j) {
        const float wj = w ? w[n * k + j] : 1.f;
        float v[8];
        Vec8<T>::load(yp + (long long)row_of[n * k + j] * E + c * 8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += wj * v[i];
      }
      if (acc) {
        float a[8];
        Vec8<T>::load(acc + n * E + c * 8, a);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += a[i];
      }
      Vec8<T>::store(y + n * E + c * 8, s);
    }
  }
}

// dgate[n,j] = dy[n] . Yp[row_of[n,j]] in fp32: one wave per assignment, xor-shuffle sum (fixed order)
template <typename T>
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ yp,
                                                              const int* __restrict__ row_of, float* __restrict__ dgate,
                                                              long long A, int E8, int k) {
  const int lane = threadIdx.x & 63;
  const long long E = (long long)E8 * 8;
  for (long long a = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); a < A; a += (long long)gridDim.x * 4) {
    const T* d = dy + (a / k) * E;
    const T* p = yp + (long long)row_of[a] * E;
    float s = 0.f;
    for (int c = lane; c < E8; c += 64) {
      float u[8], v[8];
      Vec8<T>::load(d + c * 8, u);
      Vec8<T>::load(p + c * 8, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) s += u[i] * v[i];
    }
    s = wave_sum(s);
    if (lane == 0) dgate[a] = s;
  }
}

// dl[n, e_j] = g_j * (dgate_j - sum_i g_i dgate_i), zero elsewhere, rounded once to T; one thread per token
template <typename T>
__global__ __launch_bounds__(256) void moe_route_bwd_kernel(const int* __restrict__ idx, const float* __restrict__ gate,
                                                            const float* __restrict__ dgate, T* __restrict__ dl,
                                                            long long N, int X, int k) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int j = 0; j < k; ++j) s += gate[n * k + j] * dgate[n * k + j];
  T* o = dl + n * X;
  for (int e = 0; e < X; ++e) st1<T>(o + e, 0.f);
  for (int j = 0; j < k; ++j) st1<T>(o + idx[n * k + j], gate[n * k + j] * (dgate[n * k + j] - s));
}

// out[e, :] = column sums of the live rows [off[e], off[e] + cnt[e]) of D [*, N]: a block owns 32 chunks of 8 columns
// of one expert, its 8 row lanes stride the segment and are combined through LDS in lane order (fixed order)
template <typename T>
__global__ __launch_bounds__(256) void moe_segsum_kernel(const T* __restrict__ D, const int* __restrict__ off,
                                                         const int* __restrict__ cnt, float* __restrict__ out, int N8) {
  __shared__ float red[8][32][9];
  const int e = blockIdx.y;
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const long long N = (long long)N8 * 8;
  const long long b = off[e];
  const int rows = cnt[e];
  float a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = 0.f;
  if (c < N8)
    for (int r = rl; r < rows; r += 8) {
      float v[8];
      Vec8<T>::load(D + (b + r) * N + c * 8, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] += v[i];
    }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[rl][cl][i] = a[i];
  __syncthreads();
  if (rl == 0 && c < N8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float s = 0.f;
      for (int q = 0; q < 8; ++q) s += red[q][cl][i];
      out[e * N + c * 8 + i] = s;
    }
  }
}

inline bool moe_al(const void* p, uintptr_t a) { return p && (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline unsigned moe_wave_blocks(long long rows) {
  const long long b = (rows + 3) / 4;
  return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}
inline bool moe_shape(long long N, int X, int k) {
  return N >= 1 && X >= 1 && X <= kMoeMaxX && k >= 1 && k <= kMoeMaxK && k <= X;
}

}  // namespace

// G: the row tile of the grouped GEMM; every expert's segment of the sorted buffers is padded to a multiple of it.
DL4J_API int dl4j_moe_row_tile() { return kMoeTile; }

// Rcap = roundup(N*k + X*(G-1), G): the rows of the expert-sorted buffers for N tokens (0 for arguments out of range
// or a plan beyond 32-bit rows).
DL4J_API long long dl4j_moe_rows(long long N, int k, int X) {
  if (!moe_shape(N, X, k) || N > (0x7fffffffLL / 2 - (long long)X * kMoeTile) / k) return 0;
  return (N * k + (long long)X * (kMoeTile - 1) + kMoeTile - 1) / kMoeTile * kMoeTile;
}

// int32 words of the workspace of dl4j_moe_route (the per-block histograms).
DL4J_API long long dl4j_moe_route_ws(long long N, int X) {
  return N < 1 || X < 1 ? 0 : (N + kMoeTok - 1) / kMoeTok * X;
}

// logits fp32 [N, X] -> idx [N, k], gate fp32 [N, k], cnt [X], off [X + 1], row_of [N, k], src_of [Rcap],
// tile_expert [Rcap / G] (see the top of the file), ws: dl4j_moe_route_ws(N, X) int32 words. Three launches, nothing
// read back. Returns -1 (nothing launched) for a null or misaligned (4 bytes) pointer, N < 1, X outside 1..64, k
// outside 1..min(X, 8) or a plan beyond 32-bit rows.
DL4J_API int dl4j_moe_route(const float* logits, long long N, int X, int k, int* idx, float* gate, int* cnt, int* off,
                            int* row_of, int* src_of, int* tile_expert, int* ws, hipStream_t s) {
  const long long Rcap = dl4j_moe_rows(N, k, X);
  if (Rcap < 1) return -1;
  if (!moe_al(logits, 4) || !moe_al(idx, 4) || !moe_al(gate, 4) || !moe_al(cnt, 4) || !moe_al(off, 4) ||
      !moe_al(row_of, 4) || !moe_al(src_of, 4) || !moe_al(tile_expert, 4) || !moe_al(ws, 4))
    return -1;
  const unsigned nblk = (unsigned)((N + kMoeTok - 1) / kMoeTok);
  hipLaunchKernelGGL(moe_topk_kernel, dim3(nblk), dim3(kMoeTok), 0, s, logits, N, X, k, idx, gate, ws, src_of, Rcap);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(256), 0, s, ws, (int)nblk, X, cnt, off, tile_expert,
                     (int)(Rcap / kMoeTile));
  hipLaunchKernelGGL(moe_scatter_kernel, dim3(nblk), dim3(kMoeTok), 0, s, (const int*)idx, (const int*)ws,
                     (const int*)off, N, X, k, row_of, src_of);
  return (int)hipGetLastError();
}

#define MOE_DT(CALL)                \
  do {                              \
    if (dtype == 1) { CALL(bf16); } \
    else { CALL(f16); }             \
  } while (0)

// xp [Rcap, E] <- x [N, E] by the plan: row r takes token src_of[r] / k, times scale[src_of[r]] when scale (fp32
// [N*k]) is given; pad rows of live tiles become zeros, rows of dead tiles are not written. dtype 1 bf16, 2 fp16.
// Returns -1 for another dtype, a null / misaligned operand (16 bytes for x / xp), E % 8, Rcap % G or k out of range.
DL4J_API int dl4j_moe_gather(int dtype, const void* x, const int* src_of, const int* tile_expert, const float* scale,
                             void* xp, long long Rcap, int E, int k, hipStream_t s) {
  if ((dtype != 1 && dtype != 2) || E < 8 || E % 8 || Rcap < kMoeTile || Rcap % kMoeTile || k < 1 || k > kMoeMaxK)
    return -1;
  if (!moe_al(x, 16) || !moe_al(xp, 16) || !moe_al(src_of, 4) || !moe_al(tile_expert, 4) || (scale && !moe_al(scale, 4)))
    return -1;
#define CALL(T) hipLaunchKernelGGL(moe_gather_kernel<T>, dim3(moe_wave_blocks(Rcap)), dim3(256), 0, s, (const T*)x, \
                                   src_of, tile_expert, scale, (T*)xp, Rcap, E / 8, k)
  MOE_DT(CALL);
#undef CALL
  return (int)hipGetLastError();
}

// y [N, E] = round(acc + sum_j w[n,j] * yp[row_of[n,j]]): w fp32 [N, k] or null (ones), acc [N, E] or null; acc may be
// y itself. Returns -1 as dl4j_moe_gather does, and for N < 1.
DL4J_API int dl4j_moe_combine(int dtype, const void* yp, const int* row_of, const float* w, const void* acc, void* y,
                              long long N, int E, int k, hipStream_t s) {
  if ((dtype != 1 && dtype != 2) || E < 8 || E % 8 || N < 1 || k < 1 || k > kMoeMaxK) return -1;
  if (!moe_al(yp, 16) || !moe_al(y, 16) || !moe_al(row_of, 4) || (w && !moe_al(w, 4)) || (acc && !moe_al(acc, 16)))
    return -1;
#define CALL(T) hipLaunchKernelGGL(moe_combine_kernel<T>, dim3(moe_wave_blocks(N)), dim3(256), 0, s, (const T*)yp, \
                                   row_of, w, (const T*)acc, (T*)y, N, E / 8, k)
  MOE_DT(CALL);
#undef CALL
  return (int)hipGetLastError();
}

// dgate fp32 [N, k] = dy[n] . yp[row_of[n,j]]. Returns -1 as dl4j_moe_combine does.
DL4J_API int dl4j_moe_combine_bwd(int dtype, const void* dy, const void* yp, const int* row_of, float* dgate,
                                  long long N, int E, int k, hipStream_t s) {
  if ((dtype != 1 && dtype != 2) || E < 8 || E % 8 || N < 1 || k < 1 || k > kMoeMaxK) return -1;
  if (!moe_al(dy, 16) || !moe_al(yp, 16) || !moe_al(row_of, 4) || !moe_al(dgate, 4)) return -1;
#define CALL(T) hipLaunchKernelGGL(moe_combine_bwd_kernel<T>, dim3(moe_wave_blocks(N * k)), dim3(256), 0, s, \
                                   (const T*)dy, (const T*)yp, row_of, dgate, N * k, E / 8, k)
  MOE_DT(CALL);
#undef CALL
  return (int)hipGetLastError();
}

// dl [N, X] in `dtype`: the gradient of the router logits from dgate (see the kernel). Returns -1 for another dtype, a
// null / misaligned pointer (2 bytes for dl), N < 1, X outside 1..64, k outside 1..min(X, 8).
DL4J_API int dl4j_moe_route_bwd(int dtype, const int* idx, const float* gate, const float* dgate, void* dl,
                                long long N, int X, int k, hipStream_t s) {
  if ((dtype != 1 && dtype != 2) || !moe_shape(N, X, k)) return -1;
  if (!moe_al(idx, 4) || !moe_al(gate, 4) || !moe_al(dgate, 4) || !moe_al(dl, 2)) return -1;
#define CALL(T) hipLaunchKernelGGL(moe_route_bwd_kernel<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, idx, \
                                   gate, dgate, (T*)dl, N, X, k)
  MOE_DT(CALL);
#undef CALL
  return (int)hipGetLastError();
}

// out fp32 [X, N] (4-byte aligned: usually a bias-gradient view) = per-expert column sums of the live rows of D
// [Rcap, N]; an empty expert gives zeros; fixed order, two calls give the same bits. Returns -1 for another dtype, a
// null / misaligned operand (16 bytes for D), N % 8 or X outside 1..64.
DL4J_API int dl4j_moe_segment_colsum(int dtype, const void* D, const int* off, const int* cnt, float* out, int X,
                                     int N, hipStream_t s) {
  if ((dtype != 1 && dtype != 2) || N < 8 || N % 8 || X < 1 || X > kMoeMaxX) return -1;
  if (!moe_al(D, 16) || !moe_al(off, 4) || !moe_al(cnt, 4) || !moe_al(out, 4)) return -1;
#define CALL(T) hipLaunchKernelGGL(moe_segsum_kernel<T>, dim3((N / 8 + 31) / 32, X), dim3(256), 0, s, (const T*)D, \
                                   off, cnt, out, N / 8)
  MOE_DT(CALL);
#undef CALL
  return (int)hipGetLastError();
}
