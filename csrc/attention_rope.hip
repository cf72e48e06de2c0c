// Rotary position embeddings (RoPE, Su et al. 2021) on the fused projection qkv [B, T, (H + 2*Hkv)*D] of the
// attention layers, for gfx950, bf16 or fp16, head dim D in {64, 128}. Q and K heads are rotated BEFORE they are
// stored and read, so the flash, decode, merge, gather and trim kernels run unchanged and the cache holds rotated keys.
//
// Convention (half-split pairs, the rotate_half of Llama / NeoX): for a head x of size D at position p, j in [0, D/2)
//   angle        = fp32(p) * inv_freq[j]            inv_freq[j] = fp32(theta^(-2j/D)), a device array from the host
//   out[j]       = x[j] * cos(angle) - x[j + D/2] * sin(angle)
//   out[j + D/2] = x[j + D/2] * cos(angle) + x[j] * sin(angle)
// in fp32 with the accurate sincosf (positions reach 10^5: the argument reduction matters), rounded once. inverse uses
// -angle: the transpose of the rotation, what backward applies to dQ and dK. V is never rotated.
//
//  * rope_chunk is the one body: a lane's 16-byte chunk (8 elements), the partner chunk D/2 elements away, the 8
//    frequencies of the pair -> the rotated chunk. The D/8 chunks of a head sit in consecutive lanes of one wave and
//    head bases are multiples of D/8 chunks, so the partner comes from __shfl_xor(.., D/16): no second load, and the
//    in-place write cannot race with the partner's read.
//  * attn_rope_kernel: one lane per chunk of the Q | K columns, in place; the V columns are neither read nor written.
//  * attn_rope_append_kernel: one lane per chunk of a whole row. Q and K chunks are rotated in place (a prompt of >= 64
//    tokens into an empty cache runs the flash forward on qkv, so K is rotated there too); K (rotated) and V chunks
//    also go to cache rows [pos - short[b], pos - short[b] + Tn) of kv [B, Tcap, 2*Hkv*D]: rotation and append of
//    csrc/attention_decode.hip in one launch, so a decode step gains none.
//  * attn_rope_append_fp8_kernel: one lane per 16 elements (two chunks, the partner at lane ^ D/32), the lane layout
//    of attn_kv_append_fp8_kernel: the rotated K, rounded to the 16-bit type, and V are quantised exactly as that
//    kernel quantises its input (the same amax reduction across the group's lanes, scale byte and pad bytes).
// Token (b, t) stands at pos - clamp(shortfall[b], 0, pos) + t (shortfall null: pos + t), the index of its cache row.
#include "attention_body.h"

// the 16 bytes of lane ^ mask
template <typename hb> __device__ __forceinline__ V8<hb> rope_shfl_xor(const V8<hb>& v, int mask) {
  union { V8<hb> h; int w[4]; } a, b;
  a.h = v;
#pragma unroll
  for (int k = 0; k < 4; ++k) b.w[k] = __shfl_xor(a.w[k], mask, 64);
  return b.h;
}

// x: the lane's chunk; partner: the chunk D/2 elements away; upper: x is the second half of its pairs; fr: the pairs'
// 8 frequencies; sign: +1 forward, -1 inverse. One product and one fma per element, written out (and contraction off:
// the angle is the ROUNDED fp32 product, nothing of it may fuse into sincosf's argument reduction) so that every
// caller compiles to the same arithmetic.
template <typename hb>
__device__ __forceinline__ V8<hb> rope_chunk(const V8<hb>& x, const V8<hb>& partner, bool upper, float posf,
                                             const float* __restrict__ fr, float sign) {
#pragma clang fp contract(off)
  const float4 f0 = *reinterpret_cast<const float4*>(fr), f1 = *reinterpret_cast<const float4*>(fr + 4);
  const float f[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
  const float side = upper ? sign : -sign;
  V8<hb> out;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float sn, cs;
    sincosf(posf * f[k], &sn, &cs);
    const float cross = (float)partner[k] * (sn * side);
    out[k] = tobf<hb>(fmaf((float)x[k], cs, cross));
  }
  return out;
}

__device__ __forceinline__ int rope_row_pos(const int* __restrict__ shortfall, long long b, int pos) {
  return shortfall ? pos - min(max(shortfall[b], 0), pos) : pos;
}

template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_rope_kernel(hb* __restrict__ qkv, const float* __restrict__ inv_freq,
                                                        const int* __restrict__ shortfall, long long total, int T,
                                                        int H, int Hkv, int pos, float sign) {
  constexpr int CH = D / 8;                                      // chunks per head
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;                                        // whole heads leave: total is a multiple of CH
  const int cpt = (H + Hkv) * CH;                                // Q | K chunks of a token
  const int c = (int)(i % cpt), cc = c % CH;
  const long long bt = i / cpt;                                  // b*T + t
  const int t = (int)(bt % T);
  const float posf = (float)(rope_row_pos(shortfall, bt / T, pos) + t);
  hb* p = qkv + bt * (long long)((H + 2 * Hkv) * D) + c * 8;
  const V8<hb> x = ld8(p);
  const V8<hb> y = rope_shfl_xor(x, CH / 2);
  *reinterpret_cast<V8<hb>*>(p) = rope_chunk(x, y, cc >= CH / 2, posf, inv_freq + (cc % (CH / 2)) * 8, sign);
}

template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_rope_append_kernel(hb* __restrict__ qkv, hb* __restrict__ kv,
                                                               const float* __restrict__ inv_freq,
                                                               const int* __restrict__ shortfall, long long total,
                                                               int Tn, int H, int Hkv, int pos, int Tcap) {
  constexpr int CH = D / 8;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;                                        // whole heads leave: total is a multiple of CH
  const int cpt = (H + 2 * Hkv) * CH;                            // chunks of a token: Q | K | V
  const int c = (int)(i % cpt), cc = c % CH, head = c / CH;
  const long long bt = i / cpt;                                  // b*Tn + t
  const int t = (int)(bt % Tn);
  const long long b = bt / Tn;
  const int row = rope_row_pos(shortfall, b, pos) + t;
  hb* p = qkv + bt * (long long)cpt * 8 + c * 8;
  V8<hb> x = ld8(p);
  const V8<hb> y = rope_shfl_xor(x, CH / 2);                     // every lane: V heads shuffle too and drop it
  if (head < H + Hkv) {
    x = rope_chunk(x, y, cc >= CH / 2, (float)row, inv_freq + (cc % (CH / 2)) * 8, 1.f);
    *reinterpret_cast<V8<hb>*>(p) = x;
  }
  if (head >= H)
    *reinterpret_cast<V8<hb>*>(kv + ((b * Tcap + row) * (2LL * Hkv) + (head - H)) * D + cc * 8) = x;
}

template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_rope_append_fp8_kernel(hb* __restrict__ qkv,
                                                                   unsigned char* __restrict__ kv8,
                                                                   const float* __restrict__ inv_freq,
                                                                   const int* __restrict__ shortfall, long long total,
                                                                   int Tn, int H, int Hkv, int pos, int Tcap) {
  constexpr int LPG = D / 16;                                    // lanes per head: 16 values each
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;                                        // whole heads leave: total is a multiple of LPG
  const int lpt = (H + 2 * Hkv) * LPG;                           // lanes of a token: Q | K | V
  const int l = (int)(i % lpt), c = l % LPG, head = l / LPG;
  const long long bt = i / lpt;                                  // b*Tn + t
  const int t = (int)(bt % Tn);
  const long long b = bt / Tn;
  const int row = rope_row_pos(shortfall, b, pos) + t;
  hb* p = qkv + bt * (long long)lpt * 16 + l * 16;
  V8<hb> lo = ld8(p), hi = ld8(p + 8);
  const V8<hb> plo = rope_shfl_xor(lo, LPG / 2), phi = rope_shfl_xor(hi, LPG / 2);
  if (head < H + Hkv) {
    const bool upper = c >= LPG / 2;
    const float* fr = inv_freq + (c % (LPG / 2)) * 16;
    lo = rope_chunk(lo, plo, upper, (float)row, fr, 1.f);
    hi = rope_chunk(hi, phi, upper, (float)row, fr + 8, 1.f);
    *reinterpret_cast<V8<hb>*>(p) = lo;
    *reinterpret_cast<V8<hb>*>(p + 8) = hi;
  }
  // from here on attn_kv_append_fp8_kernel (csrc/attention_decode.hip) on the rotated row, group g = head - H; the Q
  // lanes take part in the reduction of their own groups and write nothing
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
  if (head < H) return;
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
  const int g = head - H, E = Hkv * D, tail = (2 * Hkv + 15) & ~15;
  unsigned char* dst = kv8 + (b * Tcap + row) * (2LL * E + tail);
  *reinterpret_cast<uint4*>(dst + g * D + c * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  if (c == 0) {
    dst[2 * E + g] = (unsigned char)(ex + 127);
    if (g == 2 * Hkv - 1)
      for (int q = 2 * Hkv; q < tail; ++q) dst[2 * E + q] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ launch
static bool rope_shape_ok(int dt, int B, int T, int H, int Hkv, int D, int pos) {
  if (B < 1 || T < 1 || H < 1 || Hkv < 1 || H % Hkv || pos < 0 || (dt != 1 && dt != 2) || (D != 64 && D != 128))
    return false;
  if ((long long)pos + T > 0x7fffffffLL) return false;
  const long long total = (long long)B * T * (H + 2LL * Hkv) * (D / 8);          // the largest of the three grids
  return (total + 255) / 256 <= 0x7fffffffLL;
}

// dt: 1 = bf16, 2 = fp16. Rotates the Q and K columns of qkv [B, T, (H + 2*Hkv)*D] in place; token (b, t) stands at
// pos - clamp(shortfall[b], 0, pos) + t (shortfall: null, or int32 [B] on the device). inv_freq: fp32 [D/2] on the
// device. inverse != 0 rotates by -angle. -1 = unsupported dtype or head size, H % Hkv != 0, a null operand or one
// that is not 16-byte aligned.
DL4J_API int dl4j_attn_rope_dt(int dt, void* qkv, const float* inv_freq, const int* shortfall, int B, int T, int H,
                               int Hkv, int D, int pos, int inverse, hipStream_t s) {
  if (!rope_shape_ok(dt, B, T, H, Hkv, D, pos) || !qkv || !inv_freq) return -1;
  if (!attn_aligned16({qkv, inv_freq})) return -1;
  const long long total = (long long)B * T * (H + Hkv) * (D / 8);
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    hipLaunchKernelGGL((attn_rope_kernel<DD, hb>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (hb*)qkv,
                       inv_freq, shortfall, total, T, H, Hkv, pos, inverse ? -1.f : 1.f);
    return (int)hipGetLastError();
  });
}

template <bool FP8>
static int rope_append_launch(int dt, void* qkv, void* kv, const float* inv_freq, const int* shortfall, int B, int Tn,
                              int H, int Hkv, int D, int pos, int Tcap, hipStream_t s) {
  if (!rope_shape_ok(dt, B, Tn, H, Hkv, D, pos) || !qkv || !kv || !inv_freq) return -1;
  if (Tcap < 1 || Tcap % BLK || (long long)pos + Tn > Tcap) return -1;
  if (!attn_aligned16({qkv, kv, inv_freq})) return -1;
  const long long total = (long long)B * Tn * (H + 2 * Hkv) * (D / (FP8 ? 16 : 8));
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    const dim3 grid((unsigned)((total + 255) / 256));
    if constexpr (FP8)
      hipLaunchKernelGGL((attn_rope_append_fp8_kernel<DD, hb>), grid, dim3(256), 0, s, (hb*)qkv, (unsigned char*)kv,
                         inv_freq, shortfall, total, Tn, H, Hkv, pos, Tcap);
    else
      hipLaunchKernelGGL((attn_rope_append_kernel<DD, hb>), grid, dim3(256), 0, s, (hb*)qkv, (hb*)kv, inv_freq,
                         shortfall, total, Tn, H, Hkv, pos, Tcap);
    return (int)hipGetLastError();
  });
}

// One launch: dl4j_attn_rope_dt on qkv [B, Tn, (H + 2*Hkv)*D] (forward rotation) and the append of the rotated K and
// the V columns to rows [pos - shortfall[b], pos - shortfall[b] + Tn) of kv [B, Tcap, 2*Hkv*D]; bitwise what
// dl4j_attn_rope_dt followed by dl4j_attn_kv_append_ragged_gqa_dt gives. -1 as there, and for pos + Tn > Tcap or
// Tcap % 64 != 0.
DL4J_API int dl4j_attn_rope_append_dt(int dt, void* qkv, void* kv, const float* inv_freq, const int* shortfall, int B,
                                      int Tn, int H, int Hkv, int D, int pos, int Tcap, hipStream_t s) {
  return rope_append_launch<false>(dt, qkv, kv, inv_freq, shortfall, B, Tn, H, Hkv, D, pos, Tcap, s);
}

// The same into the fp8 cache kv8 [B, Tcap, 2*Hkv*D + roundup16(2*Hkv)] bytes: bitwise what dl4j_attn_rope_dt followed
// by dl4j_attn_kv_append_fp8_ragged_gqa_dt gives.
DL4J_API int dl4j_attn_rope_append_fp8_dt(int dt, void* qkv, void* kv8, const float* inv_freq, const int* shortfall,
                                          int B, int Tn, int H, int Hkv, int D, int pos, int Tcap, hipStream_t s) {
  return rope_append_launch<true>(dt, qkv, kv8, inv_freq, shortfall, B, Tn, H, Hkv, D, pos, Tcap, s);
}
