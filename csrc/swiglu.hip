// SwiGLU feed-forward gate for gfx950 on the fused projection gu [M, 2F] (gate columns [0, F), up columns [F, 2F)):
//   forward   out[M, F] = silu(g) * u,  silu(g) = g / (1 + exp(-g))
//   backward  with sig = 1 / (1 + exp(-g)):  dg = df*u*sig*(1 + g*(1 - sig)),  du = df*g*sig   -> dgu [M, 2F]
// Plain grid-stride elementwise kernels over 16-byte chunks (8 elements), fp32 arithmetic with one rounding, the
// accurate expf (exp(-g) overflows to +inf for g < -88.7, which gives silu = -0 and sig = 0: no NaN), no LDS.
#include "common.h"

// A thread walks the chunks i, i + stride, ... of the [M, F/8] chunk grid keeping (row, col) instead of dividing.
struct SwigluWalk {
  long long row;
  int col;
  long long drow;
  int dcol;
  __device__ __forceinline__ SwigluWalk(int F8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    row = i / F8;
    col = (int)(i - row * F8);
    drow = stride / F8;
    dcol = (int)(stride - drow * F8);
  }
  __device__ __forceinline__ void next(int F8) {
    row += drow;
    col += dcol;
    if (col >= F8) {
      col -= F8;
      ++row;
    }
  }
};

template <typename T>
__global__ void __launch_bounds__(256) swiglu_fwd_kernel(const T* __restrict__ gu, T* __restrict__ out, long long M,
                                                         int F8) {
  const long long F = (long long)F8 * 8;
  for (SwigluWalk w(F8); w.row < M; w.next(F8)) {
    float g[8], u[8], o[8];
    const T* p = gu + w.row * 2 * F + w.col * 8;
    Vec8<T>::load(p, g);
    Vec8<T>::load(p + F, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = g[k] / (1.f + expf(-g[k])) * u[k];
    Vec8<T>::store(out + w.row * F + w.col * 8, o);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) swiglu_bwd_kernel(const T* __restrict__ gu, const T* __restrict__ df,
                                                         T* __restrict__ dgu, long long M, int F8) {
  const long long F = (long long)F8 * 8;
  for (SwigluWalk w(F8); w.row < M; w.next(F8)) {
    float g[8], u[8], d[8], dg[8], du[8];
    const long long at = w.row * 2 * F + w.col * 8;
    Vec8<T>::load(gu + at, g);
    Vec8<T>::load(gu + at + F, u);
    Vec8<T>::load(df + w.row * F + w.col * 8, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float sig = 1.f / (1.f + expf(-g[k]));
      dg[k] = d[k] * u[k] * sig * (1.f + g[k] * (1.f - sig));
      du[k] = d[k] * g[k] * sig;
    }
    Vec8<T>::store(dgu + at, dg);
    Vec8<T>::store(dgu + at + F, du);
  }
}

static inline unsigned swiglu_blocks(long long M, int F8) {
  const long long b = (M * F8 + 255) / 256;
  return (unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}
static inline bool swiglu_al16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// dtype 0 fp32, 1 bf16, 2 fp16. gu [M, 2F] -> out [M, F]. Returns -1 for F % 8 != 0, F < 8, M < 1, an unknown dtype or
// a null / misaligned (16 bytes) operand.
DL4J_API int dl4j_swiglu_fwd(int dtype, const void* gu, void* out, long long M, long long F, hipStream_t s) {
  if (F < 8 || F % 8 != 0 || F / 8 > 0x7fffffffLL / 8 || M < 1 || !swiglu_al16(gu) || !swiglu_al16(out)) return -1;
  const int F8 = (int)(F / 8);
#define L(T) hipLaunchKernelGGL(swiglu_fwd_kernel<T>, dim3(swiglu_blocks(M, F8)), dim3(256), 0, s, (const T*)gu, \
                                (T*)out, M, F8)
  if (dtype == 1) L(bf16);
  else if (dtype == 2) L(f16);
  else if (dtype == 0) L(float);
  else return -1;
#undef L
  return (int)hipGetLastError();
}

// gu, dgu [M, 2F], df [M, F]; dgu may not alias gu (refused when they are the same buffer). Returns -1 as
// dl4j_swiglu_fwd does.
DL4J_API int dl4j_swiglu_bwd(int dtype, const void* gu, const void* df, void* dgu, long long M, long long F,
                             hipStream_t s) {
  if (F < 8 || F % 8 != 0 || F / 8 > 0x7fffffffLL / 8 || M < 1 || !swiglu_al16(gu) || !swiglu_al16(df) ||
      !swiglu_al16(dgu) || gu == dgu)
    return -1;
  const int F8 = (int)(F / 8);
#define L(T) hipLaunchKernelGGL(swiglu_bwd_kernel<T>, dim3(swiglu_blocks(M, F8)), dim3(256), 0, s, (const T*)gu, \
                                (const T*)df, (T*)dgu, M, F8)
  if (dtype == 1) L(bf16);
  else if (dtype == 2) L(f16);
  else if (dtype == 0) L(float);
  else return -1;
#undef L
  return (int)hipGetLastError();
}
