// Fused multi-head self attention (flash-style) for gfx950, bf16 or fp16 in / fp32 accumulate, head dim D in {64, 128}.
// Used by the transformer layers (BERT-base config of BASELINE.json; attention is new relative to the reference,
// SURVEY §2.6 / §5.7).
//
// Layout: Q, K, V are read in place from the fused projection output qkv[B, T, 3*E] (E = H*D; Q at column h*D,
// K at E + h*D, V at 2E + h*D), O is written to [B, T, E] and the backward writes dQ/dK/dV straight into a
// dqkv[B, T, 3*E] buffer — no permute copies around the kernels. Optional key-padding mask [B, T] (1 = keep), causal
// masking and attention-probability dropout (the DROP = true instances).
//
// Grouped-query attention (the *_gqa_dt entry points): H query heads share Hkv key/value heads, G = H / Hkv an
// integer, Ekv = Hkv*D; query head h uses kv head h / G. Layouts:
//   qkv, dqkv [B, T, E + 2*Ekv]   Q of head h at column h*D, K of kv head j at E + j*D, V at E + Ekv + j*D; dqkv is
//                                 fully written (dK / dV of a kv head are the sums over its group)
//   out, dout [B, T, E];  lse, dq_dot [B, H, T] indexed by the query head
//   dropout                       the mask stays keyed by b*H + h with the query head: the mask the multi-head kernel
//                                 draws on the input whose K / V heads are repeated G times
// Hkv = H is the layout above and runs the kernels above; Hkv < H runs the GQA = true instances of the same bodies.
// The forward and dQ results are bitwise those of the multi-head kernels on the repeated input.
//
// The kernels here only place these operands; their bodies, the wave mapping, the numerics and the dropout mask are
// in csrc/attention_body.h, shared with csrc/attention_cross.hip.
#include "attention_body.h"

// test / debug only: the keep mask [B*H, T, T] as uint8 (1 = kept), one thread per element
__global__ void __launch_bounds__(256) attn_drop_mask_kernel(unsigned char* __restrict__ out, long long total, int T,
                                                             DropArgs da) {
  const unsigned off = (unsigned)da.offset[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % T);
    const long long r = i / T;
    const int q = (int)(r % T);
    const unsigned bh = (unsigned)(r / T);
    const uint4 t = attn_drop_tile(da.seed, off, bh, (unsigned)q >> 2, (unsigned)k >> 2);
    out[i] = attn_drop_keep(attn_drop_word(t, q & 3), k & 3, da.thr) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ kernels
// Q rows and K rows are rows of the same qkv buffer (K at + E), Tq = Tk = T; dQ and dK go to the same dqkv buffer.
template <int D, typename hb, int NB, bool DROP = false>
__global__ void __launch_bounds__(256) attn_fwd_kernel(const hb* __restrict__ qkv, const float* __restrict__ mask,
                                                       hb* __restrict__ out, float* __restrict__ lse, int T, int H,
                                                       float scale2, int causal, DropArgs da) {
  const long long ld3 = 3LL * H * D;
  attn_fwd_body<D, hb, NB, DROP>(qkv, T * ld3, ld3, qkv + H * D, T * ld3, ld3, mask, out, lse, T, T, H, scale2, causal,
                                 da);
}

template <int D, typename hb, bool DROP = false>
__global__ void __launch_bounds__(256) attn_bwd_dq_kernel(const hb* __restrict__ qkv, const hb* __restrict__ dout,
                                                          const float* __restrict__ mask, const float* __restrict__ lse,
                                                          const float* __restrict__ dq_dot, hb* __restrict__ dqkv,
                                                          int T, int H, float scale2, float scale, int causal,
                                                          DropArgs da) {
  const long long ld3 = 3LL * H * D;
  attn_bwd_dq_body<D, hb, DROP>(qkv, T * ld3, ld3, qkv + H * D, T * ld3, ld3, dout, mask, lse, dq_dot, dqkv, T * ld3,
                                ld3, T, T, H, scale2, scale, causal, da);
}

template <int D, typename hb, bool DROP = false>
__global__ void __launch_bounds__(256) attn_bwd_dkdv_kernel(const hb* __restrict__ qkv,
                                                            const hb* __restrict__ dout,
                                                            const float* __restrict__ mask,
                                                            const float* __restrict__ lse,
                                                            const float* __restrict__ dq_dot,
                                                            hb* __restrict__ dqkv, int T, int H, float scale2,
                                                            float scale, int causal, DropArgs da) {
  const long long ld3 = 3LL * H * D;
  attn_bwd_dkdv_body<D, hb, DROP>(qkv, T * ld3, ld3, qkv + H * D, T * ld3, ld3, dout, mask, lse, dq_dot,
                                  dqkv + H * D, T * ld3, ld3, T, T, H, scale2, scale, causal, da);
}

// The grouped forms: qkv rows of E + 2*Ekv columns, K at + E, V Ekv after K; the dK/dV grid is over kv heads.
template <int D, typename hb, int NB, bool DROP = false>
__global__ void __launch_bounds__(256) attn_fwd_gqa_kernel(const hb* __restrict__ qkv, const float* __restrict__ mask,
                                                           hb* __restrict__ out, float* __restrict__ lse, int T, int H,
                                                           int Hkv, float scale2, int causal, DropArgs da) {
  const long long ld = (long long)(H + 2 * Hkv) * D;
  attn_fwd_body<D, hb, NB, DROP, true>(qkv, T * ld, ld, qkv + H * D, T * ld, ld, mask, out, lse, T, T, H, scale2,
                                       causal, da, H / Hkv, Hkv * D);
}

template <int D, typename hb, bool DROP = false>
__global__ void __launch_bounds__(256) attn_bwd_dq_gqa_kernel(const hb* __restrict__ qkv, const hb* __restrict__ dout,
                                                              const float* __restrict__ mask,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ dq_dot, hb* __restrict__ dqkv,
                                                              int T, int H, int Hkv, float scale2, float scale,
                                                              int causal, DropArgs da) {
  const long long ld = (long long)(H + 2 * Hkv) * D;
  attn_bwd_dq_body<D, hb, DROP, true>(qkv, T * ld, ld, qkv + H * D, T * ld, ld, dout, mask, lse, dq_dot, dqkv, T * ld,
                                      ld, T, T, H, scale2, scale, causal, da, H / Hkv, Hkv * D);
}

template <int D, typename hb, bool DROP = false>
__global__ void __launch_bounds__(256) attn_bwd_dkdv_gqa_kernel(const hb* __restrict__ qkv,
                                                                const hb* __restrict__ dout,
                                                                const float* __restrict__ mask,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ dq_dot,
                                                                hb* __restrict__ dqkv, int T, int H, int Hkv,
                                                                float scale2, float scale, int causal, DropArgs da) {
  const long long ld = (long long)(H + 2 * Hkv) * D;
  attn_bwd_dkdv_body<D, hb, DROP, true>(qkv, T * ld, ld, qkv + H * D, T * ld, ld, dout, mask, lse, dq_dot,
                                        dqkv + H * D, T * ld, ld, T, T, H, scale2, scale, causal, da, H / Hkv,
                                        Hkv * D);
}

// The sliding-window forms (the WIN = true instances of the bodies, always causal): one kernel per body for both head
// layouts, GQA = false being Hkv == H with its compile-time group size and V offset.
template <int D, typename hb, int NB, bool DROP, bool GQA>
__global__ void __launch_bounds__(256) attn_fwd_win_kernel(const hb* __restrict__ qkv, const float* __restrict__ mask,
                                                           hb* __restrict__ out, float* __restrict__ lse, int T, int H,
                                                           int Hkv, float scale2, int window, DropArgs da) {
  const long long ld = (long long)(H + 2 * Hkv) * D;
  attn_fwd_body<D, hb, NB, DROP, GQA, true>(qkv, T * ld, ld, qkv + H * D, T * ld, ld, mask, out, lse, T, T, H, scale2,
                                            1, da, H / Hkv, Hkv * D, window);
}

template <int D, typename hb, bool DROP, bool GQA>
__global__ void __launch_bounds__(256) attn_bwd_dq_win_kernel(const hb* __restrict__ qkv, const hb* __restrict__ dout,
                                                              const float* __restrict__ mask,
                                                              const float* __restrict__ lse,
                                                              float* __restrict__ dq_dot, hb* __restrict__ dqkv,
                                                              int T, int H, int Hkv, float scale2, float scale,
                                                              int window, DropArgs da) {
  const long long ld = (long long)(H + 2 * Hkv) * D;
  attn_bwd_dq_body<D, hb, DROP, GQA, true>(qkv, T * ld, ld, qkv + H * D, T * ld, ld, dout, mask, lse, dq_dot, dqkv,
                                           T * ld, ld, T, T, H, scale2, scale, 1, da, H / Hkv, Hkv * D, window,
                                           dq_dot);
}

template <int D, typename hb, bool DROP, bool GQA>
__global__ void __launch_bounds__(256) attn_bwd_dkdv_win_kernel(const hb* __restrict__ qkv,
                                                                const hb* __restrict__ dout,
                                                                const float* __restrict__ mask,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ dq_dot,
                                                                hb* __restrict__ dqkv, int T, int H, int Hkv,
                                                                float scale2, float scale, int window, DropArgs da) {
  const long long ld = (long long)(H + 2 * Hkv) * D;
  attn_bwd_dkdv_body<D, hb, DROP, GQA, true>(qkv, T * ld, ld, qkv + H * D, T * ld, ld, dout, mask, lse, dq_dot,
                                             dqkv + H * D, T * ld, ld, T, T, H, scale2, scale, 1, da, H / Hkv,
                                             Hkv * D, window);
}

// ------------------------------------------------------------------------------------------------ launch
static bool gqa_heads_ok(int H, int Hkv) { return H >= 1 && Hkv >= 1 && H % Hkv == 0; }

template <bool DROP>
static int fwd_win_dispatch(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T, int H,
                            int Hkv, int D, float scale, int window, DropArgs da, hipStream_t s) {
  if (B < 1 || T < 1 || window < 1 || window >= T || !gqa_heads_ok(H, Hkv)) return -1;
  const int W = window;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value, NB = DD == 64 ? 2 : 1;
    using hb = typename decltype(e)::type;
    const dim3 grid((T + BLK - 1) / BLK, B * H);
    if (Hkv == H)
      hipLaunchKernelGGL((attn_fwd_win_kernel<DD, hb, NB, DROP, false>), grid, dim3(256), 0, s, (const hb*)qkv, mask,
                         (hb*)out, lse, T, H, Hkv, scale * kLog2e, W, da);
    else
      hipLaunchKernelGGL((attn_fwd_win_kernel<DD, hb, NB, DROP, true>), grid, dim3(256), 0, s, (const hb*)qkv, mask,
                         (hb*)out, lse, T, H, Hkv, scale * kLog2e, W, da);
    return (int)hipGetLastError();
  });
}

// With dropout the dQ kernel computes Delta itself (csrc/attention_body.h) and leaves it in dq_dot for the dK/dV
// kernel, which therefore runs second and no pre kernel is launched; without dropout the order is the unwindowed one.
template <bool DROP, bool GQA>
static int bwd_win_launch(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                          const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int Hkv, int D,
                          float scale, int W, DropArgs da, hipStream_t s) {
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    const dim3 grid((T + BLK - 1) / BLK, B * H), gridkv((T + BLK - 1) / BLK, B * Hkv);
    auto dkdv = [&] {
      hipLaunchKernelGGL((attn_bwd_dkdv_win_kernel<DD, hb, DROP, GQA>), gridkv, dim3(256), 0, s, (const hb*)qkv,
                         (const hb*)dout, mask, lse, dq_dot, (hb*)dqkv, T, H, Hkv, scale * kLog2e, scale, W, da);
    };
    auto dq = [&] {
      hipLaunchKernelGGL((attn_bwd_dq_win_kernel<DD, hb, DROP, GQA>), grid, dim3(256), 0, s, (const hb*)qkv,
                         (const hb*)dout, mask, lse, dq_dot, (hb*)dqkv, T, H, Hkv, scale * kLog2e, scale, W, da);
    };
    if constexpr (DROP) {
      dq();
      dkdv();
    } else {
      const long long n = (long long)B * H * T;
      hipLaunchKernelGGL((attn_bwd_pre_kernel<DD, hb>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                         (const hb*)out, (const hb*)dout, dq_dot, B, T, H);
      dkdv();
      dq();
    }
    return (int)hipGetLastError();
  });
}

template <bool DROP>
static int bwd_win_dispatch(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                            const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int Hkv, int D,
                            float scale, int window, DropArgs da, hipStream_t s) {
  if (B < 1 || T < 1 || window < 1 || window >= T || !gqa_heads_ok(H, Hkv)) return -1;
  return Hkv == H ? bwd_win_launch<DROP, false>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale,
                                                window, da, s)
                  : bwd_win_launch<DROP, true>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale,
                                               window, da, s);
}

template <bool DROP>
static int fwd_dispatch(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T, int H,
                        int Hkv, int D, float scale, int causal, DropArgs da, hipStream_t s) {
  if (B < 1 || T < 1 || !gqa_heads_ok(H, Hkv)) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value, NB = DD == 64 ? 2 : 1;
    using hb = typename decltype(e)::type;
    const dim3 grid((T + BLK - 1) / BLK, B * H);
    if (Hkv == H)
      hipLaunchKernelGGL((attn_fwd_kernel<DD, hb, NB, DROP>), grid, dim3(256), 0, s, (const hb*)qkv, mask, (hb*)out,
                         lse, T, H, scale * kLog2e, causal, da);
    else
      hipLaunchKernelGGL((attn_fwd_gqa_kernel<DD, hb, NB, DROP>), grid, dim3(256), 0, s, (const hb*)qkv, mask,
                         (hb*)out, lse, T, H, Hkv, scale * kLog2e, causal, da);
    return (int)hipGetLastError();
  });
}

template <bool DROP>
static int bwd_dispatch(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                        const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int Hkv, int D, float scale,
                        int causal, DropArgs da, hipStream_t s) {
  if (B < 1 || T < 1 || !gqa_heads_ok(H, Hkv)) return -1;
  return attn_dispatch(dt, D, [&](auto d, auto e) {
    constexpr int DD = decltype(d)::value;
    using hb = typename decltype(e)::type;
    const long long n = (long long)B * H * T;
    hipLaunchKernelGGL((attn_bwd_pre_kernel<DD, hb>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       (const hb*)out, (const hb*)dout, dq_dot, B, T, H);
    const dim3 grid((T + BLK - 1) / BLK, B * H);
    if (Hkv == H) {
      hipLaunchKernelGGL((attn_bwd_dkdv_kernel<DD, hb, DROP>), grid, dim3(256), 0, s, (const hb*)qkv, (const hb*)dout,
                         mask, lse, dq_dot, (hb*)dqkv, T, H, scale * kLog2e, scale, causal, da);
      hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, hb, DROP>), grid, dim3(256), 0, s, (const hb*)qkv, (const hb*)dout,
                         mask, lse, dq_dot, (hb*)dqkv, T, H, scale * kLog2e, scale, causal, da);
    } else {
      const dim3 gridkv((T + BLK - 1) / BLK, B * Hkv);
      hipLaunchKernelGGL((attn_bwd_dkdv_gqa_kernel<DD, hb, DROP>), gridkv, dim3(256), 0, s, (const hb*)qkv,
                         (const hb*)dout, mask, lse, dq_dot, (hb*)dqkv, T, H, Hkv, scale * kLog2e, scale, causal, da);
      hipLaunchKernelGGL((attn_bwd_dq_gqa_kernel<DD, hb, DROP>), grid, dim3(256), 0, s, (const hb*)qkv,
                         (const hb*)dout, mask, lse, dq_dot, (hb*)dqkv, T, H, Hkv, scale * kLog2e, scale, causal, da);
    }
    return (int)hipGetLastError();
  });
}

// drop in [0, 1) -> thr = round(drop * 256) clamped to [0, 255]; false when drop is out of range
static bool drop_args(float drop, unsigned long long seed, const long long* offset, DropArgs* da) {
  if (!(drop >= 0.f && drop < 1.f) || !offset) return false;
  int thr = (int)(drop * 256.f + 0.5f);
  thr = thr > 255 ? 255 : thr;
  da->seed = seed;
  da->offset = offset;
  da->thr = (unsigned)thr;
  da->inv_keep = 256.f / (float)(256 - thr);
  return true;
}

// dt: 1 = bf16, 2 = fp16. qkv [B,T,3*H*D]; mask [B,T] fp32 or null; out [B,T,H*D]; lse [B,H,T] fp32.
// -1 = unsupported shape / dtype.
DL4J_API int dl4j_attn_fwd_dt(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T, int H,
                              int D, float scale, int causal, hipStream_t s) {
  return fwd_dispatch<false>(dt, qkv, mask, out, lse, B, T, H, H, D, scale, causal, DropArgs{}, s);
}

// Grouped heads (the layouts at the top of this file): qkv [B,T,(H+2*Hkv)*D]; out, lse as above. -1 also for Hkv < 1,
// H % Hkv != 0 or operands not 16-byte aligned.
DL4J_API int dl4j_attn_fwd_gqa_dt(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T,
                                  int H, int Hkv, int D, float scale, int causal, hipStream_t s) {
  if (!attn_aligned16({qkv, out})) return -1;
  return fwd_dispatch<false>(dt, qkv, mask, out, lse, B, T, H, Hkv, D, scale, causal, DropArgs{}, s);
}

// dout [B,T,H*D]; dq_dot: fp32 workspace [B,H,T]; dqkv [B,T,3*H*D] (fully written).
DL4J_API int dl4j_attn_bwd_dt(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                              const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int D, float scale,
                              int causal, hipStream_t s) {
  return bwd_dispatch<false>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, H, D, scale, causal, DropArgs{}, s);
}

// Grouped heads: qkv, dqkv [B,T,(H+2*Hkv)*D] (dqkv fully written); dq_dot, lse [B,H,T]. Status as dl4j_attn_fwd_gqa_dt.
DL4J_API int dl4j_attn_bwd_gqa_dt(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                                  const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int Hkv, int D,
                                  float scale, int causal, hipStream_t s) {
  if (!attn_aligned16({qkv, out, dout, dqkv})) return -1;
  return bwd_dispatch<false>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale, causal, DropArgs{},
                             s);
}

// The same with attention-probability dropout (drop probability in [0, 1), see the mask definition in
// csrc/attention_body.h): seed is a host scalar, offset a device pointer to the layer's step counter. lse is that of
// the undropped scores. -1 also for drop outside [0, 1) or a null offset.
DL4J_API int dl4j_attn_fwd_drop_dt(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T,
                                   int H, int D, float scale, int causal, float drop, unsigned long long seed,
                                   const long long* offset, hipStream_t s) {
  DropArgs da;
  if (!drop_args(drop, seed, offset, &da)) return -1;
  return fwd_dispatch<true>(dt, qkv, mask, out, lse, B, T, H, H, D, scale, causal, da, s);
}

DL4J_API int dl4j_attn_fwd_drop_gqa_dt(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T,
                                       int H, int Hkv, int D, float scale, int causal, float drop,
                                       unsigned long long seed, const long long* offset, hipStream_t s) {
  DropArgs da;
  if (!drop_args(drop, seed, offset, &da) || !attn_aligned16({qkv, out})) return -1;
  return fwd_dispatch<true>(dt, qkv, mask, out, lse, B, T, H, Hkv, D, scale, causal, da, s);
}

DL4J_API int dl4j_attn_bwd_drop_dt(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                                   const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int D,
                                   float scale, int causal, float drop, unsigned long long seed,
                                   const long long* offset, hipStream_t s) {
  DropArgs da;
  if (!drop_args(drop, seed, offset, &da)) return -1;
  return bwd_dispatch<true>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, H, D, scale, causal, da, s);
}

DL4J_API int dl4j_attn_bwd_drop_gqa_dt(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                                       const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int Hkv,
                                       int D, float scale, int causal, float drop, unsigned long long seed,
                                       const long long* offset, hipStream_t s) {
  DropArgs da;
  if (!drop_args(drop, seed, offset, &da) || !attn_aligned16({qkv, out, dout, dqkv})) return -1;
  return bwd_dispatch<true>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale, causal, da, s);
}

// Causal attention with a sliding window: query q sees keys q - window < k <= q (window >= 1 keys, itself included;
// Mistral's sliding_window). Operands, layouts and status codes of dl4j_attn_fwd_gqa_dt / dl4j_attn_bwd_gqa_dt with
// causal = 1 (Hkv = H is plain multi-head); key blocks no query of a tile can see are skipped. drop = 0 runs the
// kernels without dropout (seed / offset unused, offset may be null); drop in (0, 1) is that of the *_drop_* entry
// points and draws the same keep mask. A window >= T sees what the causal cut sees and runs the causal kernels
// without a window (their bits). With dropout the windowed backward takes Delta from its own probabilities instead of
// the stored output (csrc/attention_body.h) and uses dq_dot as the hand-over between its two kernels. -1 also for
// window < 1.
DL4J_API int dl4j_attn_fwd_win_dt(int dt, const void* qkv, const float* mask, void* out, float* lse, int B, int T,
                                  int H, int Hkv, int D, float scale, int window, float drop, unsigned long long seed,
                                  const long long* offset, hipStream_t s) {
  if (!attn_aligned16({qkv, out}) || window < 1) return -1;
  if (window >= T)
    return drop == 0.f ? dl4j_attn_fwd_gqa_dt(dt, qkv, mask, out, lse, B, T, H, Hkv, D, scale, 1, s)
                       : dl4j_attn_fwd_drop_gqa_dt(dt, qkv, mask, out, lse, B, T, H, Hkv, D, scale, 1, drop, seed,
                                                   offset, s);
  if (drop == 0.f)
    return fwd_win_dispatch<false>(dt, qkv, mask, out, lse, B, T, H, Hkv, D, scale, window, DropArgs{}, s);
  DropArgs da;
  if (!drop_args(drop, seed, offset, &da)) return -1;
  return fwd_win_dispatch<true>(dt, qkv, mask, out, lse, B, T, H, Hkv, D, scale, window, da, s);
}

DL4J_API int dl4j_attn_bwd_win_dt(int dt, const void* qkv, const void* out, const void* dout, const float* mask,
                                  const float* lse, float* dq_dot, void* dqkv, int B, int T, int H, int Hkv, int D,
                                  float scale, int window, float drop, unsigned long long seed,
                                  const long long* offset, hipStream_t s) {
  if (!attn_aligned16({qkv, out, dout, dqkv}) || window < 1) return -1;
  if (window >= T)
    return drop == 0.f ? dl4j_attn_bwd_gqa_dt(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale, 1, s)
                       : dl4j_attn_bwd_drop_gqa_dt(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale,
                                                   1, drop, seed, offset, s);
  if (drop == 0.f)
    return bwd_win_dispatch<false>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale, window,
                                   DropArgs{}, s);
  DropArgs da;
  if (!drop_args(drop, seed, offset, &da)) return -1;
  return bwd_win_dispatch<true>(dt, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, Hkv, D, scale, window, da, s);
}

// Test / debug only: keep [B*H, T, T] uint8 (1 = kept) of the mask the DROP kernels apply. Never part of a step.
DL4J_API int dl4j_attn_drop_mask(unsigned char* keep, int BH, int T, float drop, unsigned long long seed,
                                 const long long* offset, hipStream_t s) {
  DropArgs da;
  if (BH < 1 || T < 1 || !keep || !drop_args(drop, seed, offset, &da)) return -1;
  const long long total = (long long)BH * T * T;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(attn_drop_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, s, keep, total, T, da);
  return (int)hipGetLastError();
}

DL4J_API int dl4j_attn_fwd(const void* qkv, const float* mask, void* out, float* lse, int B, int T, int H, int D,
                           float scale, int causal, hipStream_t s) {
  return dl4j_attn_fwd_dt(1, qkv, mask, out, lse, B, T, H, D, scale, causal, s);
}

DL4J_API int dl4j_attn_bwd(const void* qkv, const void* out, const void* dout, const float* mask, const float* lse,
                           float* dq_dot, void* dqkv, int B, int T, int H, int D, float scale, int causal,
                           hipStream_t s) {
  return dl4j_attn_bwd_dt(1, qkv, out, dout, mask, lse, dq_dot, dqkv, B, T, H, D, scale, causal, s);
}
