// Speculative decoding for gfx950: the accept / reject / resample step that checks K drafted tokens against the
// target's K+1 distributions, the commit that turns the rows' new lengths into cache positions, the prompt-lookup
// (n-gram) draft and the copy that keeps an assistant's distribution. Conventions as in generation.hip: sums run in a
// fixed order, selections are by value under a total order, the only atomics are integer ones, nothing allocates or
// synchronises.
//
// ------------------------------------------------------------------------------------------------------- verify
// One block per batch row b. Target row i (i = 0 .. K) of V probabilities lies at p + i*pT + b*pB (element strides;
// contiguous in V: the output layer's [mb, V, T] is a view of time-major memory, read where it lies), draft row
// i (i < K) at q + i*qT + b*qB, or q null: the draft was deterministic, q_i is one-hot at the draft token. Draft
// token i is d[b*dB + i*dK]. With x as fp32 (NaN and negative values count as 0) the tempered distributions are the
// row sampler's: weights w = exp2((log2 x - log2 max) / temperature), p~ = wp / Sp, q~ = wq / Sq, nothing filtered.
//   for i = 0 .. K-1: accept d_i iff u_2i * q~_i(d_i) < p~_i(d_i), evaluated without a division as
//       u * wq(d) * Sp < wp(d) * Sq  (a token outside [0, V) has p = 0: rejected);
//       greedy: accept iff d_i is the argmax of p_i, the lowest index among tied maxima.
//   at the first rejection a: emit one token drawn with u_(2a+1) from r = max(0, wp * Sq - wq * Sp) (the residual
//       max(0, p~ - q~) times Sp * Sq) by the sampler's index-ordered running mass: thread c owns a contiguous run of
//       units, the running mass at index j is (the partials of the threads before c, in order) + (c's sum up to and
//       including j), the token is the first index whose running mass exceeds u * total, the last index of positive
//       mass if rounding leaves none. A residual without mass draws from wp instead. Greedy: the argmax of p_a.
//   with all K accepted: one token from wp of row K, with u_(2K+1).
// Every emitted token goes to tokens[b, cursor], log(x_token) (the raw target probability) to logps[b, cursor], and
// with ``hist`` to hist[b, len + 1 + (number emitted before it)]. The row stops after an eosToken (emitted) and
// when cursor reaches N; either marks it finished. A row that is finished on entry emits nothing, keeps len and
// cursor and gets next = padToken; every other row gets next = its last emitted token and len += tokens emitted
// (a + 1 unless it stopped early). ``next2`` (may be null) receives the same value at next2[b * next2B]: the first
// column of the target's next chunk. counters (may be null): [0] += min(K, N - cursor on entry), the drafts that
// could still be emitted, [1] += the accepted drafts that were emitted.
//   uniforms  u_s = (r >> 8) * 2^-24, r = word 0 of philox4x32_10({row, slot s, 0x53504543, offset mod 2^32},
//             {seed low, seed high}), s = 0 .. 2K+1; greedy draws nothing (u = 0). uout [mb, 2K+2] (may be null)
//             receives them. The entry point can advance the counter on the device after the call.
//
// ------------------------------------------------------------------------------------------------------- commit
// One block: maxlen = max_b len[b]; shortfall[b] = maxlen - len[b]; slot[0] = rows not finished, slot[1] = maxlen.
//
// -------------------------------------------------------------------------------------------------- n-gram draft
// One block per row, integers only. hist[b, 0 .. L], L = len[b], is the prompt and everything emitted; the last
// entry is the token not yet fed. For n = ngram .. 1 the largest j < L with hist[j-n+1 .. j] == hist[L-n+1 .. L];
// at the first n that has one, d_i = hist[j + 1 + ((i - 1) mod (L - j))], i = 1 .. K (the continuation, extended
// periodically where it runs off the end); without a match d_i = hist[L].
//
// --------------------------------------------------------------------------------------------------------- keep
// After the row sampler has drawn draft i + 1 from an assistant's output q [mb, V]: one launch copies q into row i
// of the [K, mb, V] buffer the verify kernel reads and the drawn token (the sampler writes a contiguous [mb]) into
// column i + 1 of the target's [mb, K + 1] chunk. Raw elements, 16-byte vectors where the rows allow.
#include "common.h"

static constexpr int SPEC_T = 256;                       // threads per block of every kernel here
static constexpr int SPEC_KMAX = 16;                      // drafted tokens per round
static constexpr unsigned SPEC_PHILOX_TAG = 0x53504543u;  // "SPEC"

__device__ __forceinline__ float spec_clean(float x) { return x > 0.f ? x : 0.f; }

// Rows p and q read together in units laid out by p's alignment: unit 0 is the head (the elements before p's first
// 16-byte boundary), units 1 .. nvec are 8 elements (one 16-byte load for 16-bit types, two for fp32), unit nvec + 1
// is the tail; ascending units visit ascending indices. q takes the vector loads where it shares p's alignment and
// element loads otherwise; a null q is one-hot at ``hot``.
template <typename T>
struct SpecRows {
  const T* p;
  const T* q;
  int V, hot, head, nvec, nunits;
  bool qvec;
  __device__ __forceinline__ SpecRows(const T* p_, const T* q_, int V_, int hot_) : p(p_), q(q_), V(V_), hot(hot_) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(p_) & 15) / sizeof(T));
    head = min(mis ? (int)(16 / sizeof(T)) - mis : 0, V_);
    nvec = (V_ - head) / 8;
    nunits = nvec + 2;
    qvec = q_ && ((reinterpret_cast<uintptr_t>(p_) ^ reinterpret_cast<uintptr_t>(q_)) & 15) == 0;
  }
  __device__ __forceinline__ int load(int u, float (&xp)[8], float (&xq)[8], int& base) const {
    int n;
    if (u >= 1 && u <= nvec) {
      base = head + (u - 1) * 8;
      n = 8;
      RawVec8<T> v;
      v.load(p + base);
#pragma unroll
      for (int i = 0; i < 8; ++i) xp[i] = spec_clean(v.get(i));
      if (qvec) {
        RawVec8<T> w;
        w.load(q + base);
#pragma unroll
        for (int i = 0; i < 8; ++i) xq[i] = spec_clean(w.get(i));
        return n;
      }
    } else {
      base = u == 0 ? 0 : head + nvec * 8;
      n = u == 0 ? head : V - base;
#pragma unroll
      for (int i = 0; i < 8; ++i) xp[i] = i < n ? spec_clean(ld1<T>(p + base + i)) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      xq[i] = i >= n ? 0.f : q ? spec_clean(ld1<T>(q + base + i)) : (base + i == hot ? 1.f : 0.f);
    return n;
  }
  // f(xp, xq, index) for every element of units u0, u0 + step, ... < u1, in that order
  template <typename F>
  __device__ __forceinline__ void each(int u0, int u1, int step, F f) const {
    for (int u = u0; u < u1; u += step) {
      float xp[8], xq[8];
      int base;
      const int n = load(u, xp, xq, base);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < n) f(xp[i], xq[i], base + i);
    }
  }
};

template <typename T>
__global__ void __launch_bounds__(SPEC_T) spec_verify_kernel(
    const T* __restrict__ p, long long pT, long long pB, const T* __restrict__ q, long long qT, long long qB,
    const long long* __restrict__ d, long long dB, long long dK, int K, int V, float invT, int greedy, uint2 key,
    const long long* __restrict__ offset, int* __restrict__ len, int* __restrict__ cursor,
    unsigned char* __restrict__ fin, int eos, int pad, int N, long long* __restrict__ tokens,
    float* __restrict__ logps, long long* __restrict__ next, long long* __restrict__ next2, long long next2B,
    long long* __restrict__ hist, int Hcap, int* __restrict__ counters, float* __restrict__ uout) {
  __shared__ float red[SPEC_T];
  __shared__ float red2[SPEC_T];
  __shared__ int redi[SPEC_T];
  __shared__ float su[2 * SPEC_KMAX + 2];
  __shared__ float stotal;
  __shared__ int sel[2];
  __shared__ int state[3];                                // finished on entry, cursor, len
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 2 * K + 2) {
    float u = 0.f;
    if (!greedy)
      u = u01(philox4x32_10(make_uint4((unsigned)b, (unsigned)tid, SPEC_PHILOX_TAG, (unsigned)*offset), key).x);
    su[tid] = u;
    if (uout) uout[(long long)b * (2 * K + 2) + tid] = u;
  }
  if (tid == 0) {
    state[0] = fin[b] != 0 || cursor[b] >= N || cursor[b] < 0;
    state[1] = cursor[b];
    state[2] = len[b];
  }
  __syncthreads();
  if (state[0]) {                                         // block-uniform
    if (tid == 0) {
      fin[b] = 1;
      next[b] = pad;
      if (next2) next2[(long long)b * next2B] = pad;
    }
    return;
  }
  int cur = state[1];
  const int L = state[2], cur0 = cur;
  int emitted = 0, nacc = 0, finished = 0, last = pad;
  bool stop = false;
  // everything that decides the control flow below is read from LDS after a barrier: uniform over the block
  for (int i = 0; i <= K && !stop; ++i) {
    const bool bonus = i == K;
    const T* pr = p + (long long)i * pT + (long long)b * pB;
    const long long di = bonus ? -1 : d[(long long)b * dB + (long long)i * dK];
    const int dd = (di >= 0 && di < V) ? (int)di : -1;
    const T* qr = (q && !bonus) ? q + (long long)i * qT + (long long)b * qB : nullptr;
    const SpecRows<T> R(pr, qr, V, dd);
    // ---- row maxima; p's with the lowest index among ties
    float mx = -1.f, mq = 0.f;
    int mi = 0x7fffffff;
    R.each(tid, R.nunits, SPEC_T, [&](float xp, float xq, int j) {
      if (xp > mx) { mx = xp; mi = j; }
      mq = fmaxf(mq, xq);
    });
    red[tid] = mx;
    redi[tid] = mi;
    red2[tid] = mq;
    __syncthreads();
    for (int s = SPEC_T / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const float o = red[tid + s];
        const int oi = redi[tid + s];
        if (o > red[tid] || (o == red[tid] && oi < redi[tid])) { red[tid] = o; redi[tid] = oi; }
        red2[tid] = fmaxf(red2[tid], red2[tid + s]);
      }
      __syncthreads();
    }
    const float pmax = red[0], qmax = red2[0];
    const int amax = redi[0];
    __syncthreads();
    int tok;
    bool accepted = false;
    if (greedy || !(pmax > 0.f)) {                        // an all-zero row has nothing to draw from: its argmax (0)
      accepted = greedy && !bonus && dd == amax;
      tok = amax;
    } else {
      const float lp = __log2f(pmax), lq = qmax > 0.f ? __log2f(qmax) : 0.f;
      auto wp = [&](float x) { return x > 0.f ? exp2f((__log2f(x) - lp) * invT) : 0.f; };
      auto wq = [&](float x) { return x > 0.f ? exp2f((__log2f(x) - lq) * invT) : 0.f; };
      // ---- the two masses: per-thread partials in unit order, merged by a fixed tree
      float sp = 0.f, sq = 0.f;
      R.each(tid, R.nunits, SPEC_T, [&](float xp, float xq, int) {
        sp += wp(xp);
        sq += wq(xq);
      });
      red[tid] = sp;
      red2[tid] = sq;
      __syncthreads();
      for (int s = SPEC_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
          red[tid] += red[tid + s];
          red2[tid] += red2[tid + s];
        }
        __syncthreads();
      }
      const float Sp = red[0], Sq = red2[0];
      __syncthreads();
      if (!bonus && dd >= 0) {
        const float wpd = wp(spec_clean(ld1<T>(pr + dd)));
        const float wqd = qr ? wq(spec_clean(ld1<T>(qr + dd))) : 1.f;
        accepted = su[2 * i] * wqd * Sp < wpd * Sq;
      }
      tok = dd;
      if (!accepted) {
        // ---- draw from the residual (from wp itself for the bonus token, or when the residual has no mass)
        const float u = su[2 * i + 1];
        const int uch = (R.nunits + SPEC_T - 1) / SPEC_T;
        const int u0 = min(tid * uch, R.nunits), u1 = min(u0 + uch, R.nunits);
        bool plain = bonus;
        for (;;) {
          // two rounded products and their difference, never a fused multiply-add: equal rows must leave exactly 0
          auto mass = [&](float xp, float xq) {
#pragma clang fp contract(off)
            const float a = wp(xp) * Sq, c = wq(xq) * Sp;
            return plain ? wp(xp) : fmaxf(a - c, 0.f);
          };
          float part = 0.f;
          R.each(u0, u1, 1, [&](float xp, float xq, int) { part += mass(xp, xq); });
          red[tid] = part;
          __syncthreads();
          if (tid == 0) {                                 // serial exclusive scan in thread order
            float run = 0.f;
            for (int c = 0; c < SPEC_T; ++c) {
              const float v = red[c];
              red[c] = run;
              run += v;
            }
            stotal = run;
            sel[0] = 0x7fffffff;
            sel[1] = -1;
          }
          __syncthreads();
          const float total = stotal, base = red[tid];
          if (!plain && !(total > 0.f)) {                 // block-uniform
            plain = true;
            __syncthreads();
            continue;
          }
          const float target = u * total;
          if (part > 0.f) {
            float loc = 0.f;
            int hit = 0x7fffffff, lastpos = -1;
            R.each(u0, u1, 1, [&](float xp, float xq, int j) {
              const float w = mass(xp, xq);
              if (!(w > 0.f)) return;
              loc += w;
              lastpos = j;
              if (hit == 0x7fffffff && base + loc > target) hit = j;
            });
            if (hit != 0x7fffffff) atomicMin(&sel[0], hit);
            if (lastpos >= 0) atomicMax(&sel[1], lastpos);
          }
          __syncthreads();
          tok = sel[0] != 0x7fffffff ? sel[0] : sel[1];
          if (tok < 0) tok = amax;
          __syncthreads();
          break;
        }
      }
    }
    // ---- emit
    if (tid == 0) {
      tokens[(long long)b * N + cur] = tok;
      logps[(long long)b * N + cur] = logf(spec_clean(ld1<T>(pr + tok)));
      if (hist && L + 1 + emitted >= 0 && L + 1 + emitted < Hcap) hist[(long long)b * Hcap + L + 1 + emitted] = tok;
    }
    ++cur;
    ++emitted;
    last = tok;
    if (accepted) ++nacc;
    else stop = true;
    if (eos >= 0 && tok == eos) finished = 1;
    if (cur >= N) finished = 1;
    if (finished) stop = true;
  }
  if (tid == 0) {
    cursor[b] = cur;
    len[b] = L + emitted;
    fin[b] = (unsigned char)finished;
    next[b] = last;
    if (next2) next2[(long long)b * next2B] = last;
    if (counters) {
      atomicAdd(&counters[0], min(K, N - cur0));
      atomicAdd(&counters[1], nacc);
    }
  }
}

__global__ void spec_bump_kernel(long long* __restrict__ offset) { *offset += 1; }

// ------------------------------------------------------------------------------------------------------- commit
__global__ void __launch_bounds__(SPEC_T) spec_commit_kernel(const int* __restrict__ len,
                                                             const unsigned char* __restrict__ fin, int mb,
                                                             int* __restrict__ shortfall, int* __restrict__ slot) {
  __shared__ int rmax[SPEC_T];
  __shared__ int rcnt[SPEC_T];
  const int tid = threadIdx.x;
  int m = 0, c = 0;
  for (int i = tid; i < mb; i += SPEC_T) {
    m = max(m, len[i]);
    c += fin[i] ? 0 : 1;
  }
  rmax[tid] = m;
  rcnt[tid] = c;
  __syncthreads();
  for (int s = SPEC_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      rmax[tid] = max(rmax[tid], rmax[tid + s]);
      rcnt[tid] += rcnt[tid + s];
    }
    __syncthreads();
  }
  const int maxlen = rmax[0];
  for (int i = tid; i < mb; i += SPEC_T) shortfall[i] = maxlen - len[i];
  if (tid == 0) {
    slot[0] = rcnt[0];
    slot[1] = maxlen;
  }
}

// -------------------------------------------------------------------------------------------------- n-gram draft
__global__ void __launch_bounds__(SPEC_T) spec_ngram_kernel(const long long* __restrict__ hist, int Hcap,
                                                            const int* __restrict__ len, int ngram, int K,
                                                            long long* __restrict__ d, long long dB, long long dK) {
  __shared__ int best;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long* h = hist + (long long)b * Hcap;
  const int L = min(max(len[b], 0), Hcap - 1);
  int j = -1;
  for (int n = ngram; n >= 1 && j < 0; --n) {             // j comes from LDS after a barrier: uniform
    if (tid == 0) best = -1;
    __syncthreads();
    if (L - n + 1 >= 0) {
      int m = -1;
      for (int e = n - 1 + tid; e < L; e += SPEC_T) {     // ascending: the last match of a lane is its largest
        bool same = true;
        for (int k = 0; k < n; ++k) same = same && h[e - k] == h[L - k];
        if (same) m = e;
      }
      if (m >= 0) atomicMax(&best, m);
    }
    __syncthreads();
    j = best;
    __syncthreads();
  }
  if (tid < K) d[(long long)b * dB + (long long)tid * dK] = j >= 0 ? h[j + 1 + (tid % (L - j))] : h[L];
}

// ------------------------------------------------------------------------------------------------------- keep
// dst[b*dstB + v] = src[b*V + v] (raw elements of ``esize`` bytes; 16-byte vectors where ``vec``), and with tokSrc
// tokDst[b*tokDstB] = tokSrc[b]: an assistant's distribution and the draft token drawn from it, put where the verify
// kernel and the target's chunk read them. grid (x over a row, y = b).
__global__ void __launch_bounds__(SPEC_T) spec_keep_kernel(const unsigned char* __restrict__ src,
                                                           unsigned char* __restrict__ dst, long long dstB, int V,
                                                           int esize, int vec, const long long* __restrict__ tokSrc,
                                                           long long* __restrict__ tokDst, long long tokDstB) {
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * SPEC_T + threadIdx.x;
  const unsigned char* s = src + (long long)b * V * esize;
  unsigned char* t = dst + (long long)b * dstB * esize;
  if (vec) {
    if (i < (long long)V * esize / 16) reinterpret_cast<uint4*>(t)[i] = reinterpret_cast<const uint4*>(s)[i];
  } else if (i < V) {
    if (esize == 2) reinterpret_cast<u16*>(t)[i] = reinterpret_cast<const u16*>(s)[i];
    else reinterpret_cast<unsigned*>(t)[i] = reinterpret_cast<const unsigned*>(s)[i];
  }
  if (tokSrc && blockIdx.x == 0 && threadIdx.x == 0) tokDst[(long long)b * tokDstB] = tokSrc[b];
}

// ------------------------------------------------------------------------------------------------------ launch
// dt: 0 fp32, 1 bf16, 2 fp16. p: K+1 target rows per batch row at p + i*pT + b*pB (element strides, rows contiguous
// in V); q: K draft rows addressed the same way, or null (one-hot at the draft token); d: draft token i of row b at
// d[b*dB + i*dK]. len / cursor int32 [mb] and finished uint8 [mb] are read and updated; tokens int64 [mb, N] and
// logps fp32 [mb, N] receive the emitted tokens from cursor[b] on; next int64 [mb]; next2 (or null) the same value
// at next2[b*next2B]; hist int64 [mb, Hcap] or null; counters int32 [2] or null; u fp32 [mb, 2K+2] or null.
// advance != 0 adds 1 to *offset after the draws (on the device, in stream order). Semantics at the top of this file.
// -1 = unsupported dtype, null pointer, K outside 1..16, a negative stride, mb*(K+1)*V >= 2^31 or parameters out of
// range.
DL4J_API int dl4j_spec_verify_dt(int dt, const void* p, long long pT, long long pB, const void* q, long long qT,
                                 long long qB, const long long* d, long long dB, long long dK, int mb, int K, int V,
                                 float temperature, int greedy, unsigned long long seed, long long* offset,
                                 int advance, int* len, int* cursor, unsigned char* finished, int eosToken,
                                 int padToken, int N, long long* tokens, float* logps, long long* next,
                                 long long* next2, long long next2B, long long* hist, int Hcap, int* counters,
                                 float* u, hipStream_t s) {
  if (dt < 0 || dt > 2 || !p || !d || !len || !cursor || !finished || !tokens || !logps || !next) return -1;
  if (mb < 1 || mb > 65535 * 256 || K < 1 || K > SPEC_KMAX || V < 1 || N < 1) return -1;
  if ((long long)mb * (K + 1) * V >= (1LL << 31)) return -1;
  if (pT < 0 || pB < 0 || qT < 0 || qB < 0 || dB < 0 || dK < 0 || next2B < 0) return -1;
  if (!greedy && (!offset || !(temperature > 0.f))) return -1;
  if (hist && Hcap < 1) return -1;
  const uint2 key = make_uint2((unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32));
  const float invT = greedy ? 1.f : 1.f / temperature;
#define SPEC_VERIFY(T)                                                                                                 \
  hipLaunchKernelGGL(spec_verify_kernel<T>, dim3(mb), dim3(SPEC_T), 0, s, (const T*)p, pT, pB, (const T*)q, qT, qB, d,  \
                     dB, dK, K, V, invT, greedy, key, offset, len, cursor, finished, eosToken, padToken, N, tokens,    \
                     logps, next, next2, next2B, hist, Hcap, counters, u)
  if (dt == 0) SPEC_VERIFY(float);
  else if (dt == 1) SPEC_VERIFY(bf16);
  else SPEC_VERIFY(f16);
#undef SPEC_VERIFY
  const int rc = (int)hipGetLastError();
  if (rc || greedy || !advance) return rc;
  hipLaunchKernelGGL(spec_bump_kernel, dim3(1), dim3(1), 0, s, offset);
  return (int)hipGetLastError();
}

// len int32 [mb], finished uint8 [mb] -> shortfall int32 [mb] = max(len) - len, slot int32 [2] = (rows not finished,
// max(len)). -1 = null pointer or mb < 1.
DL4J_API int dl4j_spec_commit(const int* len, const unsigned char* finished, int mb, int* shortfall, int* slot,
                              hipStream_t s) {
  if (!len || !finished || !shortfall || !slot || mb < 1) return -1;
  hipLaunchKernelGGL(spec_commit_kernel, dim3(1), dim3(SPEC_T), 0, s, len, finished, mb, shortfall, slot);
  return (int)hipGetLastError();
}

// hist int64 [mb, Hcap], len int32 [mb] (row b's history is hist[b, 0 .. len[b]], len[b] clamped below Hcap) ->
// draft token i (i = 1 .. K) of row b at d[b*dB + (i-1)*dK]. -1 = null pointer, ngram outside 1..8, K outside 1..16,
// a negative stride or mb / Hcap < 1.
DL4J_API int dl4j_spec_ngram_draft(const long long* hist, int Hcap, const int* len, int mb, int ngram, int K,
                                   long long* d, long long dB, long long dK, hipStream_t s) {
  if (!hist || !len || !d || mb < 1 || mb > 65535 * 256 || Hcap < 1) return -1;
  if (ngram < 1 || ngram > 8 || K < 1 || K > SPEC_KMAX || dB < 0 || dK < 0) return -1;
  hipLaunchKernelGGL(spec_ngram_kernel, dim3(mb), dim3(SPEC_T), 0, s, hist, Hcap, len, ngram, K, d, dB, dK);
  return (int)hipGetLastError();
}

// dst[b*dstB + v] = src[b*V + v] for b < mb, v < V (src contiguous [mb, V], dstB >= V in elements), and with tokSrc
// (int64 [mb]) tokDst[b*tokDstB] = tokSrc[b]. -1 = unsupported dtype, null pointer, sizes out of range, or a tokSrc
// without a tokDst.
DL4J_API int dl4j_spec_keep_dt(int dt, const void* src, void* dst, long long dstB, int mb, int V,
                               const long long* tokSrc, long long* tokDst, long long tokDstB, hipStream_t s) {
  if (dt < 0 || dt > 2 || !src || !dst || src == dst || mb < 1 || mb > 65535 || V < 1 || dstB < V) return -1;
  if ((long long)mb * V >= (1LL << 31) || (tokSrc && (!tokDst || tokDstB < 0))) return -1;
  const int esize = dt == 0 ? 4 : 2;
  const int vec = ((long long)V * esize) % 16 == 0 && (dstB * esize) % 16 == 0 &&
                  ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const long long n = vec ? (long long)V * esize / 16 : V;
  hipLaunchKernelGGL(spec_keep_kernel, dim3((unsigned)((n + SPEC_T - 1) / SPEC_T), mb), dim3(SPEC_T), 0, s,
                     (const unsigned char*)src, (unsigned char*)dst, dstB, V, esize, vec, tokSrc, tokDst, tokDstB);
  return (int)hipGetLastError();
}
