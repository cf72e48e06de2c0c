// Cross attention (flash-style) for gfx950: queries of one sequence (length Tq) attend over the keys / values of
// another (length Tk, its own key-padding mask). bf16 or fp16 in / fp32 accumulate, head dim D in {64, 128}.
// Used by CrossAttentionLayer and TransformerDecoderLayer (encoder-decoder transformers).
//
// Layout (the projections write it directly, a cached memory projection is passed as is):
//   q, out, dout, dq [B, Tq, E]   contiguous, head h at column h*D (E = H*D)
//   kv [B, TkCap, 2E]             K of head h at column h*D, V at E + h*D (the decode cache layout); rows [0, Tk) are
//                                 valid, rows at or beyond Tk are never loaded; the batch stride is TkCap*2E
//   dkv [B, Tk, 2E]               fully written
//   kmask [B, Tk] fp32 (1 = keep) or null;  lse, dq_dot [B, H, Tq] fp32
// There is no causal flag and no dropout instance.
//
// The kernels here only place these operands; their bodies (and the wave mapping and numerics) are those of
// csrc/attention.hip, in csrc/attention_body.h, with causal = 0 and DROP = false folded away at compile time. At
// Tq = Tk the results are those of the self-attention kernels bit for bit.
#include "attention_body.h"

// ------------------------------------------------------------------------------------------------ kernels
template <int D, typename hb, int NB>
__global__ void __launch_bounds__(256) attn_cross_fwd_kernel(const hb* __restrict__ qp, const hb* __restrict__ kv,
                                                             const float* __restrict__ kmask, hb* __restrict__ out,
                                                             float* __restrict__ lse, int Tq, int Tk, int TkCap,
                                                             int H, float scale2) {
  const long long E = H * D;
  attn_fwd_body<D, hb, NB, false>(qp, Tq * E, E, kv, TkCap * 2 * E, 2 * E, kmask, out, lse, Tq, Tk, H, scale2, 0,
                                  DropArgs{});
}

template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_cross_bwd_dq_kernel(const hb* __restrict__ qp, const hb* __restrict__ kv,
                                                                const hb* __restrict__ dout,
                                                                const float* __restrict__ kmask,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ dq_dot, hb* __restrict__ dq,
                                                                int Tq, int Tk, int TkCap, int H, float scale2,
                                                                float scale) {
  const long long E = H * D;
  attn_bwd_dq_body<D, hb, false>(qp, Tq * E, E, kv, TkCap * 2 * E, 2 * E, dout, kmask, lse, dq_dot, dq, Tq * E, E, Tq,
                                 Tk, H, scale2, scale, 0, DropArgs{});
}

template <int D, typename hb>
__global__ void __launch_bounds__(256) attn_cross_bwd_dkdv_kernel(const hb* __restrict__ qp, const hb* __restrict__ kv,
                                                                  const hb* __restrict__ dout,
                                                                  const float* __restrict__ kmask,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ dq_dot,
                                                                  hb* __restrict__ dkv, int Tq, int Tk, int TkCap,
                                                                  int H, float scale2, float scale) {
  const long long E = H * D;
  attn_bwd_dkdv_body<D, hb, false>(qp, Tq * E, E, kv, TkCap * 2 * E, 2 * E, dout, kmask, lse, dq_dot, dkv, Tk * 2 * E,
                                   2 * E, Tq, Tk, H, scale2, scale, 0, DropArgs{});
}

// ------------------------------------------------------------------------------------------------ launch
static bool cross_shape_ok(int B, int Tq, int Tk, int TkCap, int H) {
  return B >= 1 && Tq >= 1 && Tk >= 1 && H >= 1 && Tk <= TkCap && (long long)B * H <= 65535;
}

// dt: 1 = bf16, 2 = fp16. q [B,Tq,H*D]; kv [B,TkCap,2*H*D] with rows [0,Tk) valid; kmask [B,Tk] fp32 or null;
// out [B,Tq,H*D]; lse [B,H,Tq] fp32. -1 (nothing written) = unsupported dtype / head size, Tk > TkCap,
// B*H > 65535 or an operand that is not 16-byte aligned.
DL4J_API int dl4j_attn_cross_fwd_dt(int dt, const void* q, const void* kv, const float* kmask, void* out, float* lse,
                                    int B, int Tq, int Tk, int TkCap, int H, int D, float scale, hipStream_t s) {
  if (!cross_shape_ok(B, Tq, Tk, TkCap, H)) return -1;
  if (!q || !kv || !out || !lse || !attn_aligned16({q, kv, out})) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value, NB = DD == 64 ? 2 : 1;
    using hb = typename decltype(e)::type;
    hipLaunchKernelGGL((attn_cross_fwd_kernel<DD, hb, NB>), dim3((Tq + BLK - 1) / BLK, B * H), dim3(256), 0, s,
                       (const hb*)q, (const hb*)kv, kmask, (hb*)out, lse, Tq, Tk, TkCap, H, scale * kLog2e);
    return (int)hipGetLastError();
  });
}

// dout [B,Tq,H*D]; dq_dot: fp32 workspace [B,H,Tq]; dq [B,Tq,H*D] and dkv [B,Tk,2*H*D] (both fully written).
DL4J_API int dl4j_attn_cross_bwd_dt(int dt, const void* q, const void* kv, const void* out, const void* dout,
                                    const float* kmask, const float* lse, float* dq_dot, void* dq, void* dkv, int B,
                                    int Tq, int Tk, int TkCap, int H, int D, float scale, hipStream_t s) {
  if (!cross_shape_ok(B, Tq, Tk, TkCap, H)) return -1;
  if (!q || !kv || !out || !dout || !lse || !dq_dot || !dq || !dkv) return -1;
  if (!attn_aligned16({q, kv, out, dout, dq, dkv})) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    const long long n = (long long)B * H * Tq;
    hipLaunchKernelGGL((attn_bwd_pre_kernel<DD, hb>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       (const hb*)out, (const hb*)dout, dq_dot, B, Tq, H);
    hipLaunchKernelGGL((attn_cross_bwd_dkdv_kernel<DD, hb>), dim3((Tk + BLK - 1) / BLK, B * H), dim3(256), 0, s,
                       (const hb*)q, (const hb*)kv, (const hb*)dout, kmask, lse, dq_dot, (hb*)dkv, Tq, Tk, TkCap, H,
                       scale * kLog2e, scale);
    hipLaunchKernelGGL((attn_cross_bwd_dq_kernel<DD, hb>), dim3((Tq + BLK - 1) / BLK, B * H), dim3(256), 0, s,
                       (const hb*)q, (const hb*)kv, (const hb*)dout, kmask, lse, dq_dot, (hb*)dq, Tq, Tk, TkCap, H,
                       scale * kLog2e, scale);
    return (int)hipGetLastError();
  });
}
