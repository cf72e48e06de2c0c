// Fused GRU and SimpleRnn recurrences for gfx950: the whole time loop of one layer in ONE launch, forward and
// backward, with the design of the single-workgroup LSTM kernel (csrc/lstm.hip):
//   * one workgroup owns 16 minibatch rows for all T steps; rows are independent in the recurrence, so there is NO
//     inter-workgroup communication of any kind in this file: no flags, no spin-waits, no atomics, no cooperative
//     launch. A workgroup never waits for another one. H beyond one workgroup (8 waves of 16*NT units, NT <= 4,
//     so H <= 512) returns -1 and the caller runs its per-step path;
//   * each wave owns 16*NT hidden units for ALL gate blocks, so r, z, n and q of one (row, unit) sit in the same
//     lane/register of three MFMA accumulators; the gate math and the lane's own fp32 copy of h_{t-1} (the z * h
//     term) never leave registers;
//   * h_{t-1} as the MFMA A operand lives in a double-buffered LDS tile [2][16][H + pad] in the element type, one
//     __syncthreads per step; RWᵀ streams from L2 in the fragment-packed layout [n/16][k/KC][lane][FE]
//     (dl4j_rnn_pack_rw below: lstm_pack_rw_kernel generalised to a gate-block count);
//   * the next step's zx / eps / cache operands are prefetched one step ahead (not at NT = 4: register budget);
//     loads use clamped row indices, stores are predicated; rows >= mb of the last tile compute on zeros and write
//     nothing.
// The input projection zx = x·W + b for all steps and the weight gradients are library GEMMs outside.
//
// GRU (cuDNN / PyTorch convention = Keras reset_after=True; gate blocks on the 3H axis are [r | z | n]):
//   a = h_{t-1}·RW;  r = sigmoid(zx_r + a_r);  z = sigmoid(zx_z + a_z);  q = a_n + bRn;  n = tanh(zx_n + r*q)
//   h_t = ((1 - z)*n + z*h_{t-1}) * mask_t
// RNN: h_t = act(zx_t + h_{t-1}·RW) * mask_t, act = tanh or relu.
// Backward per step (dh = (eps_t + dh_next) * mask_t):
//   GRU: dzn = dh*(1-z)*(1-n²); dzz = dh*(h_{t-1}-n)*z*(1-z); dzr = dzn*q*r*(1-r);
//        dz[t] = [dzr | dzz | dzn | dzn*r] (fp32 [T, mb, 4H]: columns 0..3H are the input-side deltas, columns
//        0..2H and 3H..4H the recurrent-side ones); dh_next = dh*z + [dzr | dzz | dzn*r]·RWᵀ (one K-loop over 3H)
//   RNN: dz = dh*act'(h_t) from the stored output (tanh' = 1-h², relu' = h > 0); dh_next = dz·RWᵀ.
#include "rnn_frag.h"

enum { CELL_GRU = 0, CELL_TANH = 1, CELL_RELU = 2 };

template <int CELL> constexpr int gate_blocks() { return CELL == CELL_GRU ? 3 : 1; }

// RW fragments (16 B per lane each) issued together per load batch: about 16 forward, 8 backward at NT = 1 and 4
// above (the budget lstm.hip settled on; resource report of every instance in profiles/gru.txt: no scratch).
template <int G, int NT> constexpr int fwd_kb() {
  return 16 / (G * NT) > 8 ? 8 : (16 / (G * NT) > 0 ? 16 / (G * NT) : 1);
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int NT, int CELL>
__global__ void __launch_bounds__(512) gru_fwd_kernel(
    const T* __restrict__ zx, const T* __restrict__ rwt, const float* __restrict__ brn, const float* __restrict__ h0,
    const float* __restrict__ mask, float* __restrict__ out, T* __restrict__ out16, float* __restrict__ gates,
    float* __restrict__ hT, int Tn, int mb, int H) {
  constexpr int G = gate_blocks<CELL>();
  constexpr int KB = fwd_kb<G, NT>();                          // k-steps per load batch
  constexpr bool PF = NT < 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ld = H + row_pad<T>();
  T* hbuf = reinterpret_cast<T*>(smem);                        // [2][16][ld]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16;
  const int hb = wave * 16 * NT, hw = wave * NT, H16 = H / 16;
  const int col = lane & 15, rg = (lane >> 4) * 4;
  const int GH = G * H;
  const int KS = H / Mf<T>::KC;                                // k-steps per fragment row of the packed RWᵀ

  // h_{-1} into LDS buffer 0 (rows >= mb are zero so they contribute nothing)
  for (int i = threadIdx.x; i < 16 * H; i += blockDim.x) {
    const int r = i / H, j = i - r * H, m = m0 + r;
    hbuf[r * ld + j] = cvt<T>((h0 && m < mb) ? h0[(long long)m * H + j] : 0.f);
  }
  int mrow[4];                                                 // clamped rows: loads never branch
#pragma unroll
  for (int r = 0; r < 4; ++r) mrow[r] = min(m0 + rg + r, mb - 1);
  float h[NT][4], bq[NT];                                      // the lane's own h in fp32; bRn
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int j = hb + nt * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) h[nt][r] = (h0 && m0 + rg + r < mb) ? h0[(long long)mrow[r] * H + j] : 0.f;
    bq[nt] = (CELL == CELL_GRU && brn) ? brn[j] : 0.f;
  }
  // zx[t] / mask[t] operands, loaded one step ahead
  float zv[G][NT][4], mv[4];
  auto load_step = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long zrow = ((long long)t * mb + mrow[r]) * GH;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int j = hb + nt * 16 + col;
#pragma unroll
        for (int g = 0; g < G; ++g) zv[g][nt][r] = ld1<T>(zx + zrow + g * H + j);
      }
      mv[r] = mask ? mask[(long long)mrow[r] * Tn + t] : 1.f;
    }
  };
  if (PF) load_step(0);
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < Tn; ++t) {
    f4_t acc[G][NT];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[g][nt] = f4_t{0.f, 0.f, 0.f, 0.f};
    const T* hA = hbuf + cur * 16 * ld + col * ld;
    for (int k0 = 0; k0 < H; k0 += KB * Mf<T>::KC) {
      typename Mf<T>::frag a[KB], b[KB][G][NT];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int k = k0 + kb * Mf<T>::KC;
        if (KB == 1 || k < H) {
          a[kb] = Mf<T>::load(hA + k, lane);
#pragma unroll
          for (int g = 0; g < G; ++g)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              b[kb][g][nt] = *reinterpret_cast<const typename Mf<T>::frag*>(
                  rwt + (((long long)(g * H16 + hw + nt) * KS + k / Mf<T>::KC) * 64 + lane) * Mf<T>::FE);
        }
      }
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        if (KB == 1 || k0 + kb * Mf<T>::KC < H) {
#pragma unroll
          for (int g = 0; g < G; ++g)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[g][nt] = Mf<T>::mma(a[kb], b[kb][g][nt], acc[g][nt]);
        }
      }
    }
    if (!PF) load_step(t);
    T* hN = hbuf + (cur ^ 1) * 16 * ld;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = hb + nt * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = rg + r;
        const bool valid = m0 + rr < mb;
        float hn, gr = 0.f, gz = 0.f, gn = 0.f, gq = 0.f;
        if constexpr (CELL == CELL_GRU) {
          gr = sigm(zv[0][nt][r] + acc[0][nt][r]);
          gz = sigm(zv[1][nt][r] + acc[1][nt][r]);
          gq = acc[2][nt][r] + bq[nt];
          gn = tanh_f(zv[2][nt][r] + gr * gq);
          hn = (1.f - gz) * gn + gz * h[nt][r];
        } else {
          const float pre = zv[0][nt][r] + acc[0][nt][r];
          hn = CELL == CELL_TANH ? tanh_f(pre) : fmaxf(pre, 0.f);
        }
        hn = valid ? hn * mv[r] : 0.f;
        h[nt][r] = hn;
        hN[rr * ld + j] = cvt<T>(hn);
        if (valid) {
          const long long orow = ((long long)t * mb + m0 + rr) * H;
          out[orow + j] = hn;
          if (out16) out16[orow + j] = cvt<T>(hn);
          if constexpr (CELL == CELL_GRU) if (gates) {
            float* gp = gates + orow * 4 + j;
            gp[0] = gr;
            gp[H] = gz;
            gp[2 * H] = gn;
            gp[3 * H] = gq;
          }
        }
      }
    }
    if (PF && t + 1 < Tn) load_step(t + 1);                    // next step's HBM operands in flight now
    __syncthreads();
    cur ^= 1;
  }
  if (hT) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = hb + nt * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + rg + r;
        if (m < mb) hT[(long long)m * H + j] = h[nt][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// GRU: gates = [r | z | n | q] fp32 [T, mb, 4H], dz fp32 [T, mb, 4H] = [dzr | dzz | dzn | dzn*r].
// RNN: gates unused, dz fp32 [T, mb, H]. out = the forward's fp32 h_t [T, mb, H] (h_{t-1} of the GRU, act' of the RNN).
template <typename T, int NT, int CELL>
__global__ void __launch_bounds__(512) gru_bwd_kernel(
    const void* __restrict__ eps, int eps_dt, const float* __restrict__ gates, const float* __restrict__ out,
    const float* __restrict__ h0, const T* __restrict__ rw, const float* __restrict__ mask,
    const float* __restrict__ dh_last, float* __restrict__ dz, float* __restrict__ dh0, int Tn, int mb, int H,
    int t_end) {
  constexpr int G = gate_blocks<CELL>();
  constexpr int KB = NT == 1 ? 8 : (NT == 2 ? 2 : 1);          // k-steps per load batch
  constexpr bool PF = NT < 4;
  constexpr int NV = CELL == CELL_GRU ? 5 : 1;                 // cached values per (row, unit): r z n q h_{t-1} | h_t
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int GH = G * H;
  const int ld = GH + row_pad<T>();
  T* zb = reinterpret_cast<T*>(smem);                          // [16][ld]: the recurrent-side deltas, A operand
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16;
  const int hb = wave * 16 * NT, hw = wave * NT;
  const int col = lane & 15, rg = (lane >> 4) * 4;
  const int KS = GH / Mf<T>::KC;                               // k-steps per fragment row of the packed RW
  const int DW = CELL == CELL_GRU ? 4 * H : H;                 // row width of dz

  int mrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) mrow[r] = min(m0 + rg + r, mb - 1);
  float dhn[NT][4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int j = hb + nt * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dhn[nt][r] = (dh_last && m0 + rg + r < mb) ? dh_last[(long long)mrow[r] * H + j] : 0.f;
  }
  // step operands, prefetched one step ahead
  float ev[NT][4], cv[NV][NT][4], mv[4];
  auto load_step = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long hrow = ((long long)t * mb + mrow[r]) * H;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int j = hb + nt * 16 + col;
        ev[nt][r] = ld_any(eps, eps_dt, hrow + j);
        if constexpr (CELL == CELL_GRU) {
#pragma unroll
          for (int g = 0; g < 4; ++g) cv[g][nt][r] = gates[hrow * 4 + g * H + j];
          cv[4][nt][r] = t > 0 ? out[hrow - (long long)mb * H + j] : (h0 ? h0[(long long)mrow[r] * H + j] : 0.f);
        } else {
          cv[0][nt][r] = out[hrow + j];
        }
      }
      mv[r] = mask ? mask[(long long)mrow[r] * Tn + t] : 1.f;
    }
  };
  if (PF) load_step(Tn - 1);

  for (int t = Tn - 1; t >= t_end; --t) {
    if (!PF) load_step(t);
    float d[CELL == CELL_GRU ? 4 : 1][NT][4], carry[NT][4];    // GRU: dzr dzz dzn dzn*r
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = m0 + rg + r < mb;
        const float dh = valid ? (ev[nt][r] + dhn[nt][r]) * mv[r] : 0.f;
        if constexpr (CELL == CELL_GRU) {
          const float gr = cv[0][nt][r], gz = cv[1][nt][r], gn = cv[2][nt][r], gq = cv[3][nt][r], hp = cv[4][nt][r];
          const float dzn = dh * (1.f - gz) * (1.f - gn * gn);
          d[0][nt][r] = dzn * gq * gr * (1.f - gr);
          d[1][nt][r] = dh * (hp - gn) * gz * (1.f - gz);
          d[2][nt][r] = dzn;
          d[3][nt][r] = dzn * gr;
          carry[nt][r] = dh * gz;
        } else {
          const float hv = cv[0][nt][r];
          d[0][nt][r] = CELL == CELL_TANH ? dh * (1.f - hv * hv) : (hv > 0.f ? dh : 0.f);
          carry[nt][r] = 0.f;
        }
      }
    }
    if (PF && t - 1 >= t_end) load_step(t - 1);                // next step's HBM operands in flight now
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = hb + nt * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = rg + r;
        float* dp = dz + ((long long)t * mb + m0 + rr) * DW + j;
        const bool valid = m0 + rr < mb;
        if constexpr (CELL == CELL_GRU) {
          zb[rr * ld + j] = cvt<T>(d[0][nt][r]);
          zb[rr * ld + H + j] = cvt<T>(d[1][nt][r]);
          zb[rr * ld + 2 * H + j] = cvt<T>(d[3][nt][r]);
          if (valid) {
            dp[0] = d[0][nt][r];
            dp[H] = d[1][nt][r];
            dp[2 * H] = d[2][nt][r];
            dp[3 * H] = d[3][nt][r];
          }
        } else {
          zb[rr * ld + j] = cvt<T>(d[0][nt][r]);
          if (valid) dp[0] = d[0][nt][r];
        }
      }
    }
    __syncthreads();
    f4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f4_t{0.f, 0.f, 0.f, 0.f};
    const T* zA = zb + col * ld;
    for (int k0 = 0; k0 < GH; k0 += KB * Mf<T>::KC) {
      typename Mf<T>::frag a[KB], b[KB][NT];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int k = k0 + kb * Mf<T>::KC;
        if (k < GH) {
          a[kb] = Mf<T>::load(zA + k, lane);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            b[kb][nt] = *reinterpret_cast<const typename Mf<T>::frag*>(
                rw + (((long long)(hw + nt) * KS + k / Mf<T>::KC) * 64 + lane) * Mf<T>::FE);
        }
      }
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (k0 + kb * Mf<T>::KC < GH) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[nt] = Mf<T>::mma(a[kb], b[kb][nt], acc[nt]);
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dhn[nt][r] = acc[nt][r] + carry[nt][r];
    __syncthreads();
  }
  if (dh0) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int j = hb + nt * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + rg + r;
        if (m < mb) dh0[(long long)m * H + j] = dhn[nt][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ launch
// NT = 16-unit tiles per wave, <= 8 waves per workgroup (the kernels' __launch_bounds__(512)), so H <= 512;
// 16-bit MFMA k-steps need H % 32 == 0, fp32 ones H % 16 == 0. ops/rnn_native.py gru_supported() is the same rule.
static int pick_nt(int dtype, int H) {
  if (H < 16 || H % (dtype == 0 ? 16 : 32) != 0) return 0;
  if (H / 16 <= 8) return 1;
  if (H % 32 == 0 && H / 32 <= 8) return 2;
  if (H % 64 == 0 && H / 64 <= 8) return 4;
  return 0;
}

template <typename K>
static bool set_lds(K kern, size_t bytes) {
  if (bytes > 160 * 1024) return false;
  if (bytes > 64 * 1024)
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes) == hipSuccess;
  return true;
}

template <typename T, int NT, int CELL>
static int fwd_launch(const void* zx, const void* rwt, const float* brn, const float* h0, const float* mask, float* out,
                      void* out16, float* gates, float* hT, int Tn, int mb, int H, hipStream_t s) {
  const size_t lds = 2ull * 16 * (H + row_pad<T>()) * sizeof(T);
  auto k = gru_fwd_kernel<T, NT, CELL>;
  if (!set_lds(k, lds)) return -1;
  hipLaunchKernelGGL(k, dim3((mb + 15) / 16), dim3(64 * (H / (16 * NT))), lds, s, (const T*)zx, (const T*)rwt, brn, h0,
                     mask, out, (T*)out16, gates, hT, Tn, mb, H);
  return (int)hipGetLastError();
}

template <typename T, int NT, int CELL>
static int bwd_launch(const void* eps, int eps_dt, const float* gates, const float* out, const float* h0, const void* rw,
                      const float* mask, const float* dhl, float* dz, float* dh0, int Tn, int mb, int H, int t_end,
                      hipStream_t s) {
  const size_t lds = 16ull * (gate_blocks<CELL>() * H + row_pad<T>()) * sizeof(T);
  auto k = gru_bwd_kernel<T, NT, CELL>;
  if (!set_lds(k, lds)) return -1;
  hipLaunchKernelGGL(k, dim3((mb + 15) / 16), dim3(64 * (H / (16 * NT))), lds, s, eps, eps_dt, gates, out, h0,
                     (const T*)rw, mask, dhl, dz, dh0, Tn, mb, H, t_end);
  return (int)hipGetLastError();
}

#define RNN_NT(FN, T, CELL, ...)                          \
  do {                                                    \
    if (nt == 1) return FN<T, 1, CELL>(__VA_ARGS__);      \
    if (nt == 2) return FN<T, 2, CELL>(__VA_ARGS__);      \
    return FN<T, 4, CELL>(__VA_ARGS__);                   \
  } while (0)

#define RNN_DISPATCH(FN, CELL, ...)                       \
  do {                                                    \
    const int nt = pick_nt(dtype, H);                     \
    if (nt == 0) return -1;                               \
    if (dtype == 0) RNN_NT(FN, float, CELL, __VA_ARGS__); \
    if (dtype == 1) RNN_NT(FN, bf16, CELL, __VA_ARGS__);  \
    if (dtype == 2) RNN_NT(FN, f16, CELL, __VA_ARGS__);   \
    return -1;                                            \
  } while (0)

// All four return 0 on success, -1 when the shape/dtype is outside the kernels (the caller runs its per-step path).
// dtype: 0 fp32, 1 bf16, 2 fp16 (zx, the packed weights and out16). zx [T, mb, 3H], gates [T, mb, 4H] or null.
DL4J_API int dl4j_gru_fwd(int dtype, const void* zx, const void* rwt, const float* brn, const float* h0,
                          const float* mask, float* out, void* out16, float* gates, float* hT, int Tn, int mb, int H,
                          hipStream_t s) {
  if (Tn < 1 || mb < 1) return -1;
  RNN_DISPATCH(fwd_launch, CELL_GRU, zx, rwt, brn, h0, mask, out, out16, gates, hT, Tn, mb, H, s);
}

// eps_dt: dtype of eps (0 fp32, 1 bf16, 2 fp16), read directly. dz [T, mb, 4H] = [dzr | dzz | dzn | dzn*r].
DL4J_API int dl4j_gru_bwd(int dtype, const void* eps, int eps_dt, const float* gates, const float* out, const float* h0,
                          const void* rw, const float* mask, const float* dh_last, float* dz, float* dh0, int Tn,
                          int mb, int H, int t_end, hipStream_t s) {
  if (Tn < 1 || mb < 1 || t_end < 0 || t_end >= Tn || eps_dt < 0 || eps_dt > 2) return -1;
  RNN_DISPATCH(bwd_launch, CELL_GRU, eps, eps_dt, gates, out, h0, rw, mask, dh_last, dz, dh0, Tn, mb, H, t_end, s);
}

// act: 0 tanh, 1 relu. zx [T, mb, H].
DL4J_API int dl4j_rnn_fwd(int dtype, int act, const void* zx, const void* rwt, const float* h0, const float* mask,
                          float* out, void* out16, float* hT, int Tn, int mb, int H, hipStream_t s) {
  if (Tn < 1 || mb < 1 || act < 0 || act > 1) return -1;
  if (act == 0)
    RNN_DISPATCH(fwd_launch, CELL_TANH, zx, rwt, nullptr, h0, mask, out, out16, nullptr, hT, Tn, mb, H, s);
  RNN_DISPATCH(fwd_launch, CELL_RELU, zx, rwt, nullptr, h0, mask, out, out16, nullptr, hT, Tn, mb, H, s);
}

DL4J_API int dl4j_rnn_bwd(int dtype, int act, const void* eps, int eps_dt, const float* out, const void* rw,
                          const float* mask, const float* dh_last, float* dz, float* dh0, int Tn, int mb, int H,
                          int t_end, hipStream_t s) {
  if (Tn < 1 || mb < 1 || t_end < 0 || t_end >= Tn || act < 0 || act > 1 || eps_dt < 0 || eps_dt > 2) return -1;
  if (act == 0)
    RNN_DISPATCH(bwd_launch, CELL_TANH, eps, eps_dt, nullptr, out, nullptr, rw, mask, dh_last, dz, dh0, Tn, mb, H,
                 t_end, s);
  RNN_DISPATCH(bwd_launch, CELL_RELU, eps, eps_dt, nullptr, out, nullptr, rw, mask, dh_last, dz, dh0, Tn, mb, H, t_end,
               s);
}

// ------------------------------------------------------------------------------------------ recurrent weight packing
// lstm_pack_rw_kernel (csrc/lstm_glue.hip) for G gate blocks: RW is the [H, G*H] weight view with element strides
// (s0, s1); for an [N, K] matrix m the packed image is [N/16][K/KC][4][16][FE] with KC = 4*FE (FE = 8 for 16-bit T,
// 4 for fp32).   forward: m[n][k] = RW[k][n], N = G*H, K = H      backward: m[n][k] = RW[n][k], N = H, K = G*H
template <typename T>
__global__ __launch_bounds__(256) void rnn_pack_rw_kernel(const T* __restrict__ rw, long long s0, long long s1, int H,
                                                          int G, T* __restrict__ fwd, T* __restrict__ bwd) {
  constexpr int FE = sizeof(T) == 2 ? 8 : 4, KC = 4 * FE;
  const long long total = (long long)G * H * H;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    long long q = o / FE;
    const int e = (int)(o % FE);
    const int n16 = (int)(q % 16); q /= 16;
    const int sub = (int)(q % 4); q /= 4;
    if (fwd) {
      const int KBn = H / KC;
      const int kb = (int)(q % KBn), nb = (int)(q / KBn);
      const int n = nb * 16 + n16, k = kb * KC + sub * FE + e;
      fwd[o] = rw[(long long)k * s0 + (long long)n * s1];
    }
    if (bwd) {
      const int KBn = G * H / KC;
      const int kb = (int)(q % KBn), nb = (int)(q / KBn);
      const int n = nb * 16 + n16, k = kb * KC + sub * FE + e;
      bwd[o] = rw[(long long)n * s0 + (long long)k * s1];
    }
  }
}

// dt: 0 fp32, 1 bf16, 2 fp16; G = gate blocks (3 GRU, 1 RNN). fwd / bwd may each be null.
DL4J_API int dl4j_rnn_pack_rw(int dt, const void* rw, long long s0, long long s1, int H, int G, void* fwd, void* bwd,
                              hipStream_t s) {
  if (G < 1 || G > 4 || pick_nt(dt, H) == 0) return -1;
  const long long total = (long long)G * H * H;
  const unsigned g = (unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  if (dt == 1)
    hipLaunchKernelGGL(rnn_pack_rw_kernel<bf16>, dim3(g), dim3(256), 0, s, (const bf16*)rw, s0, s1, H, G, (bf16*)fwd,
                       (bf16*)bwd);
  else if (dt == 2)
    hipLaunchKernelGGL(rnn_pack_rw_kernel<f16>, dim3(g), dim3(256), 0, s, (const f16*)rw, s0, s1, H, G, (f16*)fwd,
                       (f16*)bwd);
  else if (dt == 0)
    hipLaunchKernelGGL(rnn_pack_rw_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)rw, s0, s1, H, G, (float*)fwd,
                       (float*)bwd);
  else
    return -1;
  return (int)hipGetLastError();
}
