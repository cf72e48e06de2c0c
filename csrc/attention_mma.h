// Fragment helpers of the attention kernel bodies (csrc/attention_body.h): the v_mfma_f32_16x16x32_{bf16,f16}
// wrappers, the LDS / register fragment loads that match its operand layout, the cross-group reductions of the
// transposed-score online softmax, and the cooperative 64-row block loads into LDS.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f4_t;
template <typename T> using V8 = T __attribute__((ext_vector_type(8)));
template <typename T> using V4 = T __attribute__((ext_vector_type(4)));

static constexpr int BLK = 64;             // rows (queries or keys) per block
static constexpr float kLog2e = 1.4426950408889634f;
static constexpr float kNegInf = -INFINITY;

// v_mfma_f32_16x16x32_{bf16,f16}: same fragment layout for both element types
__device__ __forceinline__ f4_t mma(V8<__bf16> a, V8<__bf16> b, f4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f4_t mma(V8<_Float16> a, V8<_Float16> b, f4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
template <typename hb> __device__ __forceinline__ hb tobf(float v) { return (hb)v; }

// fragment of 8 hb from a row-major LDS/global row (16-byte aligned)
template <typename hb> __device__ __forceinline__ V8<hb> ld8(const hb* p) { return *reinterpret_cast<const V8<hb>*>(p); }
// two 4-element pieces (keys 4h..4h+3 and 16+4h..16+4h+3 of a 32-key step) of a transposed row
template <typename hb> __device__ __forceinline__ V8<hb> ld4x2(const hb* row, int h) {
  const V4<hb> a = *reinterpret_cast<const V4<hb>*>(row + 4 * h);
  const V4<hb> b = *reinterpret_cast<const V4<hb>*>(row + 16 + 4 * h);
  return V8<hb>{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
// B fragment from two accumulator tiles (16 rows each) in the permuted k order matching ld4x2
template <typename hb> __device__ __forceinline__ V8<hb> pack2(const f4_t& x, const f4_t& y) {
  return V8<hb>{(hb)x[0], (hb)x[1], (hb)x[2], (hb)x[3], (hb)y[0], (hb)y[1], (hb)y[2], (hb)y[3]};
}

__device__ __forceinline__ float wmax16(float v) {            // max over the 4 lane groups (l>>4)
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float wsum16(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// cooperative block loads: rows [r0, r0+64) of a [T, ld] matrix slice (D columns at col0) into LDS
template <int D, typename hb>
__device__ __forceinline__ void stage_rows(hb* dst, int dld, const hb* src, long long src_ld, int r0, int T) {
  constexpr int CPR = D / 8;                                  // 16-byte chunks per row
  for (int i = threadIdx.x; i < BLK * CPR; i += blockDim.x) {
    const int r = i / CPR, c = i - r * CPR;
    V8<hb> v;
    if (r0 + r < T) v = *reinterpret_cast<const V8<hb>*>(src + (long long)(r0 + r) * src_ld + c * 8);
    else v = V8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<V8<hb>*>(dst + r * dld + c * 8) = v;
  }
}
template <int D, typename hb>
__device__ __forceinline__ void stage_rows_t(hb* dst, int dld, const hb* src, long long src_ld, int r0, int T) {
  constexpr int CPR = D / 8;                                  // transposed: dst[d][row]
  for (int i = threadIdx.x; i < BLK * CPR; i += blockDim.x) {
    const int r = i % BLK, c = i / BLK;
    V8<hb> v;
    if (r0 + r < T) v = *reinterpret_cast<const V8<hb>*>(src + (long long)(r0 + r) * src_ld + c * 8);
    else v = V8<hb>{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[(c * 8 + k) * dld + r] = v[k];
  }
}
