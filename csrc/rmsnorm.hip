// RMSNorm forward / backward for gfx950, with the pre-norm residual add fused in, both ways:
//   s = x (+ r, rounded to T and stored);  y = s * rstd * gamma,  rstd = 1/sqrt(mean(s^2) + eps)
// The layout of csrc/layernorm.hip: one wave per row, 16-byte vector loads (8 elements per lane per chunk), the row
// held in registers, the fp32 sum of squares by wave shuffles, no LDS and no block barrier in the forward. Saves rstd
// (fp32, per row) for the backward.
// Backward: xhat = s*rstd, dxh = dy*gamma; dx = rstd*(dxh - xhat*mean(dxh*xhat)) (+ dres, the gradient arriving over
// the residual path, added in fp32 before the one rounding); dgamma (and optionally the column sums of the rounded
// dx, the producing projection's bias gradient) are accumulated per wave in registers, summed per block through LDS
// into one partial row per block and reduced by a second small kernel in a fixed order (no atomics: deterministic).
#include "common.h"

template <typename T> __device__ __forceinline__ float rms_round(float v) { return v; }
template <> __device__ __forceinline__ float rms_round<bf16>(float v) { return bf2f(f2bf(v)); }
template <> __device__ __forceinline__ float rms_round<f16>(float v) { return (float)(f16)v; }

// CH = 8-element chunks per lane (N <= 512*CH). RES: s = round_T(x + r) is written to s_out and is what the
// statistics and y are computed from (the stored value is what the backward reads), so the call is bitwise "add,
// round, then the kernel without r". x, r and s_out may alias: every element is read and written by the same lane.
template <typename T, int CH, bool RES>
__global__ void __launch_bounds__(256) rms_fwd_kernel(const T* x, const T* r, const float* __restrict__ gamma,
                                                      T* __restrict__ y, T* s_out, float* __restrict__ rstd_out,
                                                      long long M, int N, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nch = N >> 3;
  float v[CH][8];
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      Vec8<T>::load(x + row * N + ch * 8, v[c]);
      if (RES) {
        float rr[8];
        Vec8<T>::load(r + row * N + ch * 8, rr);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[c][k] += rr[k];
        Vec8<T>::store(s_out + row * N + ch * 8, v[c]);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[c][k] = rms_round<T>(v[c][k]);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) q += v[c][k] * v[c][k];
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / N + eps);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      float g[8], o[8];
      Vec8<float>::load(gamma + ch * 8, g);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = v[c][k] * rstd * g[k];
      Vec8<T>::store(y + row * N + ch * 8, o);
    }
  }
  if (lane == 0) rstd_out[row] = rstd;
}

// W waves per block, wave w takes rows r0 + w, r0 + w + W, ... of the block's row range; the W per-wave partials are
// summed through LDS so each block writes one [NP][N] partial row (NP = 1: dgamma; DS: also the column sums of the
// rounded dx). dres and dx may alias (same lane reads and writes an element).
template <typename T, int CH, int W, bool DS>
__global__ void __launch_bounds__(64 * W) rms_bwd_block(const T* __restrict__ dy, const T* __restrict__ s,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ rstd_in, const T* dres, T* dx,
                                                        float* __restrict__ part, long long M, int N, long long rpb) {
  constexpr int NP = DS ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) float lsum[];     // [W][NP][N]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = N >> 3;
  float dg[CH][8], g[CH][8], dsum[DS ? CH : 1][8];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = lane + c * 64;
#pragma unroll
    for (int k = 0; k < 8; ++k) dg[c][k] = 0.f;
    if (DS) {
#pragma unroll
      for (int k = 0; k < 8; ++k) dsum[DS ? c : 0][k] = 0.f;
    }
    if (ch < nch) Vec8<float>::load(gamma + ch * 8, g[c]);
  }
  const long long r0 = (long long)blockIdx.x * rpb;
  long long r1 = r0 + rpb;
  if (r1 > M) r1 = M;
  for (long long row = r0 + wave; row < r1; row += W) {
    const float rstd = rstd_in[row];
    float sv[CH][8], dv[CH][8], rv[CH][8];
#pragma unroll
    for (int c = 0; c < CH; ++c) {                      // all of the row's loads in flight before any use
      const int ch = lane + c * 64;
      if (ch < nch) {
        Vec8<T>::load(s + row * N + ch * 8, sv[c]);
        Vec8<T>::load(dy + row * N + ch * 8, dv[c]);
        if (dres) Vec8<T>::load(dres + row * N + ch * 8, rv[c]);
      }
    }
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (lane + c * 64 < nch) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float xh = sv[c][k] * rstd;
          const float d = dv[c][k] * g[c][k];
          sv[c][k] = xh;
          s2 += d * xh;
          dg[c][k] += dv[c][k] * xh;
          dv[c][k] = d;
        }
      }
    }
    const float m2 = wave_sum(s2) / N;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = lane + c * 64;
      if (ch < nch) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = rstd * (dv[c][k] - sv[c][k] * m2);
        if (dres) {
#pragma unroll
          for (int k = 0; k < 8; ++k) o[k] += rv[c][k];
        }
        Vec8<T>::store(dx + row * N + ch * 8, o);
        if (DS) {
          // sum what was stored (rounded to T), so the bias gradient matches a column sum of the stored dx
#pragma unroll
          for (int k = 0; k < 8; ++k) dsum[DS ? c : 0][k] += rms_round<T>(o[k]);
        }
      }
    }
  }
  float* mine = lsum + (long long)wave * NP * N;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      Vec8<float>::store(mine + ch * 8, dg[c]);
      if (DS) Vec8<float>::store(mine + N + ch * 8, dsum[DS ? c : 0]);
    }
  }
  __syncthreads();
  float* out = part + (long long)blockIdx.x * NP * N;
  for (int j = threadIdx.x; j < NP * N; j += 64 * W) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) t += lsum[w * NP * N + j];
    out[j] = t;
  }
}

// out[NP][N] = sum over the P partial rows, in a fixed order. Block = 32 columns x 8 row groups (coalesced 128-byte
// row reads), eight independent row loads per trip, the 8 group sums combined through LDS.
__global__ void __launch_bounds__(256) rms_bwd_reduce(const float* __restrict__ part, int P, int N,
                                                      float* __restrict__ dgamma, float* __restrict__ dsum, int NP) {
  __shared__ float red[8][33];
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + cl;                          // over the concatenated [dgamma (| dsum)]
  float t = 0.f;
  if (j < NP * N) {
    for (int p0 = rg; p0 < P; p0 += 64) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = p0 + 8 * u;
        v[u] = p < P ? part[(long long)p * NP * N + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) t += v[u];
    }
  }
  red[rg][cl] = t;
  __syncthreads();
  if (rg == 0 && j < NP * N) {
    float a = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) a += red[g][cl];
    (j < N ? dgamma : dsum)[j < N ? j : j - N] = a;
  }
}

// The block geometry of the LayerNorm backward: up to 128 blocks of W waves (W from the row width), at least one row
// per wave.
static constexpr int kRmsCap = 128;
template <int CH> struct RmsWaves { static constexpr int W = CH <= 2 ? 8 : (CH == 4 ? 4 : 2); };

template <typename T, int CH>
static int rms_fwd_l(const void* x, const void* r, const float* g, void* y, void* s_out, float* rstd, long long M,
                     int N, float eps, hipStream_t s) {
  const dim3 grid((unsigned)((M + 3) / 4));
  if (r)
    hipLaunchKernelGGL((rms_fwd_kernel<T, CH, true>), grid, dim3(256), 0, s, (const T*)x, (const T*)r, g, (T*)y,
                       (T*)s_out, rstd, M, N, eps);
  else
    hipLaunchKernelGGL((rms_fwd_kernel<T, CH, false>), grid, dim3(256), 0, s, (const T*)x, (const T*)nullptr, g,
                       (T*)y, (T*)nullptr, rstd, M, N, eps);
  return (int)hipGetLastError();
}

template <typename T, int CH>
static int rms_bwd_l(const void* dy, const void* sx, const float* g, const float* rstd, const void* dres, void* dx,
                     float* part, float* dgamma, float* dsum, long long M, int N, hipStream_t s) {
  constexpr int W = RmsWaves<CH>::W;
  long long blocks = (M + W - 1) / W;
  blocks = blocks > kRmsCap ? kRmsCap : blocks;
  const long long rpb = (M + blocks - 1) / blocks;
  const int NP = dsum ? 2 : 1;
  const size_t lds = (size_t)W * NP * N * sizeof(float);         // <= 64 KB: W * N <= 8192
  if (dsum)
    hipLaunchKernelGGL((rms_bwd_block<T, CH, W, true>), dim3((unsigned)blocks), dim3(64 * W), lds, s, (const T*)dy,
                       (const T*)sx, g, rstd, (const T*)dres, (T*)dx, part, M, N, rpb);
  else
    hipLaunchKernelGGL((rms_bwd_block<T, CH, W, false>), dim3((unsigned)blocks), dim3(64 * W), lds, s, (const T*)dy,
                       (const T*)sx, g, rstd, (const T*)dres, (T*)dx, part, M, N, rpb);
  hipLaunchKernelGGL(rms_bwd_reduce, dim3((NP * N + 31) / 32), dim3(256), 0, s, part, (int)blocks, N, dgamma, dsum,
                     NP);
  return (int)hipGetLastError();
}

#define RMS_CH_DISPATCH(FN, T, ...)                      \
  do {                                                   \
    if (N <= 512) return FN<T, 1>(__VA_ARGS__);          \
    if (N <= 1024) return FN<T, 2>(__VA_ARGS__);         \
    if (N <= 2048) return FN<T, 4>(__VA_ARGS__);         \
    return FN<T, 8>(__VA_ARGS__);                        \
  } while (0)

static inline bool rms_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool rms_al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// Rows of the fp32 workspace of dl4j_rms_bwd: part holds dl4j_rms_partial_rows(M) * 2 * N floats.
DL4J_API long long dl4j_rms_partial_rows(long long M) { return M < 1 ? 0 : (M < kRmsCap ? M : kRmsCap); }

// dtype 0 fp32, 1 bf16, 2 fp16. x, y [M, N]; gamma [N] fp32; rstd [M] fp32 (saved for the backward). r == null:
// y = x * rsqrt(mean(x^2) + eps) * gamma and s_out must be null. With r [M, N]: s = round_T(x + r) is written to
// s_out [M, N] (which may alias x or r) and y / rstd are computed from it. Returns -1 for N % 8 != 0, N > 4096,
// M < 1, an unknown dtype, a null or misaligned operand (16 bytes for the [M, N] operands, 4 for the fp32 vectors:
// gamma is usually a view into the flat parameters), or s_out given without r (or r without s_out).
DL4J_API int dl4j_rms_fwd(int dtype, const void* x, const void* r, const float* gamma, void* y, void* s_out,
                          float* rstd, long long M, int N, float eps, hipStream_t s) {
  if (N < 8 || N % 8 != 0 || N > 4096 || M < 1 || dtype < 0 || dtype > 2) return -1;
  if (!x || !gamma || !y || !rstd || (r == nullptr) != (s_out == nullptr)) return -1;
  if (!rms_al16(x) || !rms_al16(r) || !rms_al4(gamma) || !rms_al16(y) || !rms_al16(s_out) || !rms_al4(rstd))
    return -1;
  if (dtype == 1) RMS_CH_DISPATCH(rms_fwd_l, bf16, x, r, gamma, y, s_out, rstd, M, N, eps, s);
  if (dtype == 2) RMS_CH_DISPATCH(rms_fwd_l, f16, x, r, gamma, y, s_out, rstd, M, N, eps, s);
  RMS_CH_DISPATCH(rms_fwd_l, float, x, r, gamma, y, s_out, rstd, M, N, eps, s);
}

// dy, s (what the forward normalised: x, or its s_out), dx [M, N]; gamma, dgamma [N] fp32; rstd [M] fp32 from the
// forward. dres (optional, [M, N]): added to dx in fp32 before the one rounding; dx may alias it. dsum (optional, [N]
// fp32): column sums of the rounded dx. part: fp32 workspace of dl4j_rms_partial_rows(M) * 2 * N floats. Returns -1
// as dl4j_rms_fwd does.
DL4J_API int dl4j_rms_bwd(int dtype, const void* dy, const void* sx, const float* gamma, const float* rstd,
                          const void* dres, void* dx, float* part, float* dgamma, float* dsum, long long M, int N,
                          hipStream_t s) {
  if (N < 8 || N % 8 != 0 || N > 4096 || M < 1 || dtype < 0 || dtype > 2) return -1;
  if (!dy || !sx || !gamma || !rstd || !dx || !part || !dgamma) return -1;
  if (!rms_al16(dy) || !rms_al16(sx) || !rms_al4(gamma) || !rms_al16(dres) || !rms_al16(dx) || !rms_al16(part) ||
      !rms_al4(rstd) || !rms_al4(dgamma) || !rms_al4(dsum))
    return -1;
  if (dtype == 1) RMS_CH_DISPATCH(rms_bwd_l, bf16, dy, sx, gamma, rstd, dres, dx, part, dgamma, dsum, M, N, s);
  if (dtype == 2) RMS_CH_DISPATCH(rms_bwd_l, f16, dy, sx, gamma, rstd, dres, dx, part, dgamma, dsum, M, N, s);
  RMS_CH_DISPATCH(rms_bwd_l, float, dy, sx, gamma, rstd, dres, dx, part, dgamma, dsum, M, N, s);
}
