// MFMA fragment scheme and gate math shared by the whole-sequence recurrent kernels (lstm.hip, gru.hip).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f4_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;

template <typename T> struct Mf;
// bf16: one MFMA covers k = 32; lane l holds A[l&15][8(l>>4)+j], B[8(l>>4)+j][l&15], j = 0..7.
template <> struct Mf<bf16> {
  static constexpr int KC = 32, FE = 8;
  typedef bf16x8_t frag;
  static __device__ __forceinline__ frag load(const bf16* p, int lane) {
    return *reinterpret_cast<const frag*>(p + 8 * (lane >> 4));
  }
  static __device__ __forceinline__ f4_t mma(frag a, frag b, f4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
// fp16: same fragment shapes as bf16 on v_mfma_f32_16x16x32_f16.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8m_t;
template <> struct Mf<f16> {
  static constexpr int KC = 32, FE = 8;
  typedef f16x8m_t frag;
  static __device__ __forceinline__ frag load(const f16* p, int lane) {
    return *reinterpret_cast<const frag*>(p + 8 * (lane >> 4));
  }
  static __device__ __forceinline__ f4_t mma(frag a, frag b, f4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
// fp32: four 16x16x4 MFMAs cover k = 16; lane group h = l>>4 supplies k = 4h + j for MFMA j (the same permuted
// k order on A and B, so the sum is exact f32 fma chains).
template <> struct Mf<float> {
  static constexpr int KC = 16, FE = 4;
  typedef f4_t frag;
  static __device__ __forceinline__ frag load(const float* p, int lane) {
    return *reinterpret_cast<const frag*>(p + 4 * (lane >> 4));
  }
  static __device__ __forceinline__ f4_t mma(frag a, frag b, f4_t c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
  }
};

template <typename T> __device__ __forceinline__ T cvt(float v);
template <> __device__ __forceinline__ float cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 cvt<bf16>(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ f16 cvt<f16>(float v) { return (f16)v; }

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  // tanh via exp: accurate to a few ulp in fp32, saturates cleanly for |x| large
  const float e = __expf(-2.f * fabsf(x));
  const float r = (1.f - e) / (1.f + e);
  return copysignf(r, x);
}

template <typename T> constexpr int row_pad() { return 16 / (int)sizeof(T); }
