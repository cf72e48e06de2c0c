// Token generation for gfx950: a row sampler (greedy / temperature / top-k / top-p), a beam-search step and the
// key/value-cache row gather that follows it. Every kernel is deterministic: sums run in a fixed order (per-thread
// partials in a fixed element order, merged in a fixed tree or a serial scan), selections are by value under a total
// order, and the only atomics are integer LDS counts.
//
// ---------------------------------------------------------------------------------------------------- row sampler
// p [R, V] holds PROBABILITIES (the row softmax of RnnOutputLayer) in fp32, bf16 or fp16; 16-bit rows are read as
// they are. A block owns a row. With x_i = p_i as fp32 (NaN and negative values count as 0):
//   weights   w_i = exp2((log2 x_i - log2 max_j x_j) / temperature) in fp32, so the row maximum has weight 1;
//             x_i = 0 gives w_i = 0.
//   top-k     (k >= 1; 0 = off) keeps every i with x_i >= the k-th largest value of the row (counted with
//             multiplicity, as a sort would); ties at that value are all kept. k >= V keeps all.
//   top-p     (0 < topP <= 1; 1 = off) among the top-k survivors, M their total weight: keeps every i with
//             x_i >= t, t the largest value for which the weight of {x_i >= t} is >= topP * M. w is monotone in x,
//             so this is the threshold on the weights; ties at t are all kept and the row maximum always is.
//             t is found by a radix search (4 bits a pass) on the integer key of x — the bit pattern of a
//             non-negative float orders like the float — each pass summing per-thread bins, merged by a fixed
//             butterfly within a wave and then in wave order.
//   draw      u = (r >> 8) * 2^-24 in [0, 1), r = word 0 of
//             philox4x32_10({row, 0, 0x47454E53, offset mod 2^32}, {seed low, seed high}),
//             offset read from device memory (the PhiloxStream convention); the entry point can advance it on the
//             device after the draw, so a generation loop needs no host op per step.
//             Thread c of 512 owns a contiguous index range (a run of 8-element units, see GenRow; with top-k on and
//             at most 1024 survivors, a run of the survivors gathered in index order); its partial is the sum of
//             its kept weights in index order, the running mass at index i is
//             (sum of the partials of threads < c, in order) + (thread c's sum up to and including i), and keptMass
//             is that running mass at the last index. The token is the first kept index whose running mass exceeds
//             u * keptMass (the last kept index of positive weight if rounding leaves none).
//   outputs   tok[r] int64, logp[r] = log(x_tok) fp32, optionally u[r].
//   finished  (uint8 [R], may be null) a finished row gets padToken and log-prob 0; a row whose token equals eosToken
//             (-1 = none) is marked finished. count (may be null) receives the number of unfinished rows, summed in a
//             fixed order by a second one-block launch.
//   greedy    argmax with the lowest index among tied maxima; no Philox call, u[r] = 0.
//
// ------------------------------------------------------------------------------------------------------ beam step
// p [B*W, V], score [B, W] fp32, finished [B, W] uint8, length [B, W] int32; W in 1..16 (instantiated for 2, 4, 8,
// 16 so a thread's best-W list has compile-time indices). A block owns a batch group. Candidates: for a live beam w
// one per v with score[b, w] + log p[b*W + w, v] (log 0 = -inf), for a finished beam the single (w, padToken) with
// its score unchanged. The W best under the total order (score descending, flat index w*V + v ascending) are written
// best first — the order makes the result independent of how threads tile the candidates: parent [B, W] int32 (the
// global row b*W + w), token [B, W] int64, and score / finished / length updated in place (finished: the parent's
// flag or token == eosToken; length: the parent's, +1 if the parent was live). count as above.
//
// The sequence of a final beam is read back by gen_backtrack_kernel from the per-step parent / token rows.
//
// --------------------------------------------------------------------------------------------------- cache gather
// dst[i, 0:L, :] = src[parent[i], 0:L, :] for src [mbS, TcapS, C], dst [mbD, TcapD, C], in 16-byte vectors; parent is
// int32 in device memory (an entry outside [0, mbS) writes nothing). Rows at or beyond L of dst are not written.
// Never in place (src == dst is refused): a swap of two rows would read what it has just overwritten.
#include "common.h"

static constexpr int GEN_T = 256;                       // threads per block of the beam step and the count
static constexpr unsigned GEN_PHILOX_TAG = 0x47454E53u;  // "GENS"

// ----------------------------------------------------------------------------------------------------- helpers
// probability as fp32 with NaN / negative -> 0 (also -0.0f, whose bit pattern would not order)
__device__ __forceinline__ float gen_clean(float x) { return x > 0.f ? x : 0.f; }
__device__ __forceinline__ unsigned gen_key(float x) { return __float_as_uint(x); }

// the tail launch of a step: the unfinished count (count may be null) and the step counter's advance (may be null),
// both plain stores of one thread, ordered after the step's kernel by the stream
__global__ void __launch_bounds__(GEN_T) gen_count_kernel(const unsigned char* __restrict__ fin, int n,
                                                          int* __restrict__ count, long long* __restrict__ advance) {
  __shared__ int red[GEN_T];
  if (advance && threadIdx.x == 0) *advance += 1;
  if (!count) return;
  int c = 0;
  for (int i = threadIdx.x; i < n; i += GEN_T) c += fin[i] ? 0 : 1;
  red[threadIdx.x] = c;
  __syncthreads();
  for (int s = GEN_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = red[0];
}

// ----------------------------------------------------------------------------------------------------- row access
// A row is read in units: unit 0 is the head (the elements before the first 16-byte boundary, none when the row is
// aligned), units 1 .. nvec are vectors of 8 elements (one 16-byte load for 16-bit types, two for fp32) and unit
// nvec + 1 is the tail. Units are in index order, so a thread that visits units in ascending order visits indices in
// ascending order, whatever the row's alignment (rows of an odd V start misaligned).
template <typename T>
struct GenRow {
  const T* p;
  int V, head, nvec, nunits;
  __device__ __forceinline__ GenRow(const T* p_, int V_) : p(p_), V(V_) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(p_) & 15) / sizeof(T));
    head = min(mis ? (int)(16 / sizeof(T)) - mis : 0, V_);
    nvec = (V_ - head) / 8;
    nunits = nvec + 2;
  }
  // -> number of elements of unit u (0 .. 8), x[] their cleaned values, base the index of the first
  __device__ __forceinline__ int load(int u, float (&x)[8], int& base) const {
    if (u >= 1 && u <= nvec) {
      base = head + (u - 1) * 8;
      RawVec8<T> v;
      v.load(p + base);
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = gen_clean(v.get(i));
      return 8;
    }
    base = u == 0 ? 0 : head + nvec * 8;
    const int n = u == 0 ? head : V - base;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = i < n ? gen_clean(ld1<T>(p + base + i)) : 0.f;
    return n;
  }
};
// f(x, index) for every element of units u0, u0 + step, ... < u1, in that order
template <typename T, typename F>
__device__ __forceinline__ void gen_units(const GenRow<T>& row, int u0, int u1, int step, F f) {
  for (int u = u0; u < u1; u += step) {
    float x[8];
    int base;
    const int n = row.load(u, x, base);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < n) f(x[i], base + i);
  }
}

// The top-k survivors gathered into LDS in index order: a unit is one (value, index) entry.
struct GenCompact {
  const float* x;
  const int* idx;
  int nunits;
};
template <typename F>
__device__ __forceinline__ void gen_units(const GenCompact& c, int u0, int u1, int step, F f) {
  for (int u = u0; u < u1; u += step) f(c.x[u], c.idx[u]);
}

// ----------------------------------------------------------------------------------------------------- sampler
static constexpr int SAMP_T = 512;                       // threads per block of the sampler
static constexpr int SAMP_CAP = 1024;                    // top-k survivors kept in LDS (more: the row is re-read)

template <typename T>
__global__ void __launch_bounds__(SAMP_T) gen_sample_kernel(const T* __restrict__ p, int V, float invT, int topK,
                                                            float topP, int greedy, uint2 key,
                                                            const long long* __restrict__ offset,
                                                            long long* __restrict__ tok, float* __restrict__ logp,
                                                            float* __restrict__ uout, unsigned char* __restrict__ fin,
                                                            int eos, int pad) {
  __shared__ float red[SAMP_T];
  __shared__ int redi[SAMP_T];
  __shared__ float bins[16 * SAMP_T];
  __shared__ int hist[256];
  __shared__ int sel[2];
  __shared__ float cx[SAMP_CAP];
  __shared__ int ci[SAMP_CAP];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (fin && fin[row]) {                                 // block-uniform
    if (tid == 0) {
      tok[row] = pad;
      logp[row] = 0.f;
      if (uout) uout[row] = 0.f;
    }
    return;
  }
  const GenRow<T> R(p + (long long)row * V, V);
  // ---- row maximum, lowest index among ties (order-independent)
  float mx = -1.f;
  int mi = 0x7fffffff;
  gen_units(R, tid, R.nunits, SAMP_T, [&](float x, int i) {
    if (x > mx) { mx = x; mi = i; }                      // ascending i per thread: the first hit is the lowest
  });
  red[tid] = mx;
  redi[tid] = mi;
  __syncthreads();
  for (int s = SAMP_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const float o = red[tid + s];
      const int oi = redi[tid + s];
      if (o > red[tid] || (o == red[tid] && oi < redi[tid])) { red[tid] = o; redi[tid] = oi; }
    }
    __syncthreads();
  }
  const float pmax = red[0];
  const int amax = redi[0];
  __syncthreads();
  if (greedy || !(pmax > 0.f)) {                         // an all-zero row has nothing to draw from: its argmax (0)
    if (tid == 0) {
      tok[row] = amax;
      logp[row] = logf(pmax);
      if (uout) uout[row] = 0.f;
      if (fin && eos >= 0 && amax == eos) fin[row] = 1;
    }
    return;
  }
  const float lmax = __log2f(pmax);
  auto weight = [&](float x) { return x > 0.f ? exp2f((__log2f(x) - lmax) * invT) : 0.f; };

  // ---- top-k: key of the k-th largest value, by radix select (8 bits a pass, integer LDS counts)
  unsigned thr = 0;
  if (topK >= 1 && topK < V) {
    unsigned prefix = 0;
    int want = topK;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      if (tid == 0) { sel[0] = 0; sel[1] = want; }
      __syncthreads();
      gen_units(R, tid, R.nunits, SAMP_T, [&](float x, int) {
        const unsigned k = gen_key(x);
        if (shift == 24 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255], 1);
      });
      __syncthreads();
      // suffix counts by a parallel scan (integers: any order gives the same sums): redi[d] = sum of hist[d ..]
      const int hv = tid < 256 ? hist[tid] : 0;
      if (tid < 256) redi[tid] = hv;
      __syncthreads();
      for (int off = 1; off < 256; off <<= 1) {
        const int add = (tid < 256 && tid + off < 256) ? redi[tid + off] : 0;
        __syncthreads();
        if (tid < 256) redi[tid] += add;
        __syncthreads();
      }
      if (tid < 256) {                                   // the digit whose range of ranks holds the wanted one
        const int incl = redi[tid], excl = incl - hv;
        if (excl < want && want <= incl) { sel[0] = tid; sel[1] = want - excl; }
      }
      __syncthreads();
      prefix |= (unsigned)sel[0] << shift;
      want = sel[1];
      __syncthreads();
    }
    thr = prefix;
  }

  // ---- a few top-k survivors: gather them (value, index) into LDS in index order; top-p and the draw then run on
  // that list instead of passing over the row again. Thread c counts and then writes its contiguous run of units.
  const int rch = (R.nunits + SAMP_T - 1) / SAMP_T;
  const int r0 = min(tid * rch, R.nunits), r1 = min(r0 + rch, R.nunits);
  int ncomp = -1;
  if (thr > 0) {
    int cnt = 0;
    gen_units(R, r0, r1, 1, [&](float x, int) { cnt += gen_key(x) >= thr ? 1 : 0; });
    redi[tid] = cnt;
    __syncthreads();
    if (tid == 0) {                                      // serial exclusive scan in thread order
      int run = 0;
      for (int c = 0; c < SAMP_T; ++c) {
        const int v = redi[c];
        redi[c] = run;
        run += v;
      }
      sel[0] = run;
    }
    __syncthreads();
    const int total = sel[0];
    if (total <= SAMP_CAP) {                             // block-uniform
      int o = redi[tid];
      gen_units(R, r0, r1, 1, [&](float x, int i) {
        if (gen_key(x) >= thr) {
          cx[o] = x;
          ci[o] = i;
          ++o;
        }
      });
      ncomp = total;
    }
    __syncthreads();
  }

  auto select = [&](const auto& S) {
    // ---- top-p among the survivors
    if (topP < 1.f) {
      float m = 0.f;
      gen_units(S, tid, S.nunits, SAMP_T, [&](float x, int) {
        if (gen_key(x) >= thr) m += weight(x);
      });
      __syncthreads();
      red[tid] = m;
      __syncthreads();
      for (int s = SAMP_T / 2; s > 0; s >>= 1) {             // fixed tree
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      const float target = topP * red[0];
      unsigned prefix = 0;
      float above = 0.f;                                   // weight of the keys above the current prefix range
      for (int shift = 28; shift >= 0; shift -= 4) {
#pragma unroll
        for (int b = 0; b < 16; ++b) bins[b * SAMP_T + tid] = 0.f;
        gen_units(S, tid, S.nunits, SAMP_T, [&](float x, int) {
          const unsigned k = gen_key(x);
          if (k >= thr && (shift == 28 || (k >> (shift + 4)) == (prefix >> (shift + 4))))
            bins[((k >> shift) & 15) * SAMP_T + tid] += weight(x);
        });
        // per-thread bins -> per-wave sums by the fixed xor butterfly, -> block sums in wave order
        float bw[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) bw[b] = wave_sum(bins[b * SAMP_T + tid]);
        __syncthreads();
        if ((tid & 63) == 0) {
#pragma unroll
          for (int b = 0; b < 16; ++b) bins[b * SAMP_T + (tid >> 6)] = bw[b];
        }
        __syncthreads();
        int d = 15;
        float acc = above;
        for (; d > 0; --d) {                               // every thread reads the same sums: uniform
          float bsum = 0.f;
#pragma unroll
          for (int wv = 0; wv < SAMP_T / 64; ++wv) bsum += bins[d * SAMP_T + wv];
          if (acc + bsum >= target) break;
          acc += bsum;
        }
        above = acc;
        prefix |= (unsigned)d << shift;
        __syncthreads();
      }
      if (prefix > thr) thr = prefix;
    }

    // ---- draw: index-ordered running mass over contiguous runs of units
    const int uch = (S.nunits + SAMP_T - 1) / SAMP_T;
    const int u0 = min(tid * uch, S.nunits), u1 = min(u0 + uch, S.nunits);
    float part = 0.f;
    gen_units(S, u0, u1, 1, [&](float x, int) {
      if (gen_key(x) >= thr) part += weight(x);
    });
    __syncthreads();
    red[tid] = part;
    __syncthreads();
    if (tid == 0) {                                        // serial exclusive scan in thread order
      float run = 0.f;
      for (int c = 0; c < SAMP_T; ++c) {
        const float v = red[c];
        red[c] = run;
        run += v;
      }
      const uint4 r = philox4x32_10(make_uint4((unsigned)row, 0u, GEN_PHILOX_TAG, (unsigned)*offset), key);
      bins[0] = run;                                       // keptMass
      bins[1] = u01(r.x);
      sel[0] = 0x7fffffff;
      sel[1] = -1;
    }
    __syncthreads();
    const float kept = bins[0], u = bins[1], target = u * kept;
    const float base = red[tid];
    // the run whose running mass first exceeds the target holds the token; later runs may also see an index, so
    // the lowest wins (integer LDS min), and the last index of positive weight is the fallback
    if (part > 0.f) {
      float loc = 0.f;
      int hit = 0x7fffffff, last = -1;
      gen_units(S, u0, u1, 1, [&](float x, int i) {
        if (gen_key(x) < thr) return;
        const float w = weight(x);
        if (!(w > 0.f)) return;
        loc += w;
        last = i;
        if (hit == 0x7fffffff && base + loc > target) hit = i;
      });
      if (hit != 0x7fffffff) atomicMin(&sel[0], hit);
      if (last >= 0) atomicMax(&sel[1], last);
    }
    __syncthreads();
  };
  if (ncomp >= 0) select(GenCompact{cx, ci, ncomp});
  else select(R);
  if (tid == 0) {
    const float u = bins[1];
    int t = sel[0] != 0x7fffffff ? sel[0] : sel[1];
    if (t < 0) t = amax;
    tok[row] = t;
    logp[row] = logf(gen_clean(ld1<T>(R.p + t)));
    if (uout) uout[row] = u;
    if (fin && eos >= 0 && t == eos) fin[row] = 1;
  }
}

// ----------------------------------------------------------------------------------------------------- beam step
struct GenCand {
  float s;
  int idx;
};
__device__ __forceinline__ bool gen_better(float s, int idx, const GenCand& o) {
  return s > o.s || (s == o.s && idx < o.idx);
}
// insert into a list sorted best first (compile-time indices: stays in registers)
template <int WT>
__device__ __forceinline__ void gen_insert(GenCand (&l)[WT], float s, int idx) {
  if (!gen_better(s, idx, l[WT - 1])) return;
  l[WT - 1] = GenCand{s, idx};
#pragma unroll
  for (int j = WT - 1; j > 0; --j) {
    if (gen_better(l[j].s, l[j].idx, l[j - 1])) {
      const GenCand t = l[j - 1];
      l[j - 1] = l[j];
      l[j] = t;
    }
  }
}

template <int WT, typename T>
__global__ void __launch_bounds__(GEN_T) gen_beam_kernel(const T* __restrict__ p, int W, int V,
                                                         float* __restrict__ score, unsigned char* __restrict__ fin,
                                                         int* __restrict__ length, int* __restrict__ parent,
                                                         long long* __restrict__ token, int eos, int pad) {
  __shared__ GenCand lists[GEN_T * WT];
  __shared__ float s_old[16];
  __shared__ int f_old[16], l_old[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < W) {
    s_old[tid] = score[b * W + tid];
    f_old[tid] = fin[b * W + tid];
    l_old[tid] = length[b * W + tid];
  }
  __syncthreads();
  GenCand l[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) l[j] = GenCand{-INFINITY, 0x7fffffff};
  for (int w = 0; w < W; ++w) {
    const float sw = s_old[w];
    if (f_old[w]) {
      if (tid == (w & (GEN_T - 1))) gen_insert<WT>(l, sw, w * V + min(max(pad, 0), V - 1));
      continue;
    }
    const GenRow<T> R(p + ((long long)b * W + w) * V, V);
    gen_units(R, tid, R.nunits, GEN_T, [&](float x, int v) {
      gen_insert<WT>(l, sw + (x > 0.f ? logf(x) : -INFINITY), w * V + v);
    });
  }
#pragma unroll
  for (int j = 0; j < WT; ++j) lists[tid * WT + j] = l[j];
  __syncthreads();
  for (int s = GEN_T / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const GenCand o = lists[(tid + s) * WT + j];
        gen_insert<WT>(l, o.s, o.idx);
      }
#pragma unroll
      for (int j = 0; j < WT; ++j) lists[tid * WT + j] = l[j];
    }
    __syncthreads();
  }
  if (tid < W) {
    const GenCand c = lists[tid];                        // thread 0's list, best first
    const int w = min(c.idx / V, W - 1), v = c.idx - (c.idx / V) * V;
    const bool pf = f_old[w] != 0;
    const int t = pf ? pad : v;
    parent[b * W + tid] = b * W + w;
    token[b * W + tid] = t;
    score[b * W + tid] = c.s;
    fin[b * W + tid] = (pf || (eos >= 0 && t == eos)) ? 1 : 0;
    length[b * W + tid] = l_old[w] + (pf ? 0 : 1);
  }
}

// ----------------------------------------------------------------------------------------------------- gather
// one thread per 16-byte chunk: i = (row * L + l) * CC + c
__global__ void __launch_bounds__(256) gen_gather_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                         const int* __restrict__ parent, long long total, int L,
                                                         int CC, int mbS, int TcapS, int TcapD) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % CC);
  const long long rl = i / CC;
  const int l = (int)(rl % L);
  const long long r = rl / L;
  const int pr = parent[r];
  if (pr < 0 || pr >= mbS) return;
  dst[(r * TcapD + l) * CC + c] = src[((long long)pr * TcapS + l) * CC + c];
}

// ----------------------------------------------------------------------------------------------------- backtrack
// the sequence of the chosen final beam: one thread per example follows the parents back from row b*W + best[b]
__global__ void __launch_bounds__(256) gen_backtrack_kernel(const long long* __restrict__ toks,
                                                            const int* __restrict__ parents,
                                                            const long long* __restrict__ best,
                                                            long long* __restrict__ out, int B, int W, int N) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long rows = (long long)B * W;
  long long r = (long long)b * W + min(max(best[b], 0LL), (long long)W - 1);
  for (int t = N - 1; t >= 0; --t) {
    out[(long long)b * N + t] = toks[t * rows + r];
    const int pr = parents[t * rows + r];
    r = min(max(pr, b * W), b * W + W - 1);              // a parent is a row of the same group
  }
}

// ------------------------------------------------------------------------------------------------- step commit
// The end of one pinned generation step (nn/generation.py): every row's shortfall against the pinned capacity drops
// by one (not below 0), so the next step's ragged append / attention / embedding run one position further with the
// same launch arguments; with ``step`` the token and log-probability the sampler staged are filed as row *step of
// the [N, rows] result buffers (nothing once *step >= N). The counter is read here by every thread and bumped by
// gen_commit_bump_kernel, the next launch on the stream, so no thread can see the new value.
__global__ void __launch_bounds__(256) gen_commit_kernel(int* __restrict__ shortfall, int mb,
                                                         const int* __restrict__ step,
                                                         const long long* __restrict__ stok,
                                                         const float* __restrict__ slogp,
                                                         long long* __restrict__ tokens, float* __restrict__ logps,
                                                         int rows, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (shortfall && i < mb) shortfall[i] = max(shortfall[i] - 1, 0);
  if (step && i < rows) {
    const int t = *step;
    if (t >= 0 && t < N) {
      tokens[(long long)t * rows + i] = stok[i];
      logps[(long long)t * rows + i] = slogp[i];
    }
  }
}

__global__ void gen_commit_bump_kernel(int* __restrict__ step, int N) {
  const int t = *step;
  if (t >= 0 && t < N) *step = t + 1;
}

// ------------------------------------------------------------------------------------------------------ launch
static int gen_count_l(const unsigned char* fin, int n, int* count, long long* advance, hipStream_t s) {
  if (!count && !advance) return (int)hipGetLastError();
  hipLaunchKernelGGL(gen_count_kernel, dim3(1), dim3(GEN_T), 0, s, fin, n, count, advance);
  return (int)hipGetLastError();
}

// dt: 0 fp32, 1 bf16, 2 fp16. p [R, V] probabilities; tok [R] int64; logp [R] fp32; u [R] fp32 or null;
// finished [R] uint8 or null (count then needs it); count: int32 word or null; advance != 0 adds 1 to *offset after
// the draw (on the device, in stream order), so consecutive steps draw fresh numbers without a host op. Semantics at
// the top of this file.
// -1 = unsupported dtype, null pointer, R*V >= 2^31 or parameters out of range.
DL4J_API int dl4j_gen_sample_dt(int dt, const void* p, int R, int V, float temperature, int topK, float topP,
                                int greedy, unsigned long long seed, long long* offset, int advance, long long* tok,
                                float* logp, float* u, unsigned char* finished, int eosToken, int padToken, int* count,
                                hipStream_t s) {
  if (dt < 0 || dt > 2 || !p || !tok || !logp || R < 1 || V < 1 || (long long)R * V >= (1LL << 31)) return -1;
  if (!greedy && (!offset || !(temperature > 0.f) || topK < 0 || !(topP > 0.f) || topP > 1.f)) return -1;
  if (count && !finished) return -1;
  if (R > 65535 * 256) return -1;
  const uint2 key = make_uint2((unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32));
  const float invT = greedy ? 1.f : 1.f / temperature;
#define GEN_SAMPLE(T)                                                                                                  \
  hipLaunchKernelGGL(gen_sample_kernel<T>, dim3(R), dim3(SAMP_T), 0, s, (const T*)p, V, invT, topK, topP, greedy, key,  \
                     offset, tok, logp, u, finished, eosToken, padToken)
  if (dt == 0) GEN_SAMPLE(float);
  else if (dt == 1) GEN_SAMPLE(bf16);
  else GEN_SAMPLE(f16);
#undef GEN_SAMPLE
  const int rc = (int)hipGetLastError();
  return rc ? rc : gen_count_l(finished, R, count, (advance && !greedy) ? offset : nullptr, s);
}

template <typename T>
static void gen_beam_l(const void* p, int B, int W, int V, float* score, unsigned char* fin, int* length, int* parent,
                       long long* token, int eos, int pad, hipStream_t s) {
#define GEN_BEAM(WT)                                                                                                   \
  hipLaunchKernelGGL((gen_beam_kernel<WT, T>), dim3(B), dim3(GEN_T), 0, s, (const T*)p, W, V, score, fin, length,      \
                     parent, token, eos, pad)
  if (W <= 2) GEN_BEAM(2);
  else if (W <= 4) GEN_BEAM(4);
  else if (W <= 8) GEN_BEAM(8);
  else GEN_BEAM(16);
#undef GEN_BEAM
}

// p [B*W, V]; score [B, W] fp32, finished [B, W] uint8 and length [B, W] int32 are read and updated in place;
// parent [B, W] int32 and token [B, W] int64 are written, best beam first. -1 = W outside 1..16, W*V >= 2^31,
// B*W*V >= 2^31, unsupported dtype or null pointer.
DL4J_API int dl4j_gen_beam_step_dt(int dt, const void* p, int B, int W, int V, float* score, unsigned char* finished,
                                   int* length, int* parent, long long* token, int eosToken, int padToken, int* count,
                                   hipStream_t s) {
  if (dt < 0 || dt > 2 || !p || !score || !finished || !length || !parent || !token) return -1;
  if (B < 1 || B > 65535 * 256 || W < 1 || W > 16 || V < 1) return -1;
  if ((long long)W * V >= (1LL << 31) || (long long)B * W * V >= (1LL << 31)) return -1;
  if (dt == 0) gen_beam_l<float>(p, B, W, V, score, finished, length, parent, token, eosToken, padToken, s);
  else if (dt == 1) gen_beam_l<bf16>(p, B, W, V, score, finished, length, parent, token, eosToken, padToken, s);
  else gen_beam_l<f16>(p, B, W, V, score, finished, length, parent, token, eosToken, padToken, s);
  const int rc = (int)hipGetLastError();
  return rc ? rc : gen_count_l(finished, B * W, count, nullptr, s);
}

// dst[i, 0:L, :] = src[parent[i], 0:L, :], i < mbD; elemBytes 1 (the fp8 key/value cache's byte rows), 2 or 4; C*elemBytes must be a multiple of 16 and both
// buffers 16-byte aligned. -1 = refused (also src == dst, L beyond a capacity, null pointer).
DL4J_API int dl4j_gen_cache_gather(const void* src, void* dst, const int* parent, int mbS, int mbD, int TcapS,
                                   int TcapD, int L, int C, int elemBytes, hipStream_t s) {
  if (!src || !dst || !parent || src == dst || (elemBytes != 1 && elemBytes != 2 && elemBytes != 4)) return -1;
  if (mbS < 1 || mbD < 1 || C < 1 || L < 0 || L > TcapS || L > TcapD) return -1;
  if (((long long)C * elemBytes) & 15) return -1;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) return -1;
  if (L == 0) return 0;
  const int CC = C * elemBytes / 16;
  const long long total = (long long)mbD * L * CC;
  if ((total + 255) / 256 > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(gen_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint4*)src,
                     (uint4*)dst, parent, total, L, CC, mbS, TcapS, TcapD);
  return (int)hipGetLastError();
}

// out[b, t] = the token at step t of the beam that ends as beam best[b] of example b: toks [N, B*W] int64 and
// parents [N, B*W] int32 (global rows) as the beam steps wrote them, best [B] int64, out [B, N] int64.
// -1 = null pointer or a size outside the 32-bit index range.
DL4J_API int dl4j_gen_beam_backtrack(const long long* toks, const int* parents, const long long* best, long long* out,
                                     int B, int W, int N, hipStream_t s) {
  if (!toks || !parents || !best || !out || B < 1 || W < 1 || W > 16 || N < 1) return -1;
  if ((long long)B * W * N >= (1LL << 31)) return -1;
  hipLaunchKernelGGL(gen_backtrack_kernel, dim3((B + 255) / 256), dim3(256), 0, s, toks, parents, best, out, B, W, N);
  return (int)hipGetLastError();
}

// One pinned generation step's bookkeeping, with constant arguments: shortfall[b] = max(shortfall[b] - 1, 0) for
// b < mb (shortfall: int32 [mb], or null with mb == 0: off); with ``step`` (a device int32 word, null = off) the
// staged stok int64 [rows] / slogp fp32 [rows] go to tokens[*step, :] / logps[*step, :] of the [N, rows] buffers and
// *step becomes *step + 1; nothing is written and the counter stays once *step >= N.
// -1 = nothing to do, a shortfall without rows, a record part with a null pointer or rows / N < 1.
DL4J_API int dl4j_gen_step_commit(int* shortfall, int mb, int* step, const long long* stok, const float* slogp,
                                  long long* tokens, float* logps, int rows, int N, hipStream_t s) {
  if (!shortfall && !step) return -1;
  if (shortfall ? mb < 1 : mb != 0) return -1;
  if (step && (!stok || !slogp || !tokens || !logps || rows < 1 || N < 1)) return -1;
  if (!step) rows = 0;
  const int n = mb > rows ? mb : rows;
  hipLaunchKernelGGL(gen_commit_kernel, dim3((n + 255) / 256), dim3(256), 0, s, shortfall, mb, step, stok, slogp,
                     tokens, logps, rows, N);
  const int rc = (int)hipGetLastError();
  if (rc || !step) return rc;
  hipLaunchKernelGGL(gen_commit_bump_kernel, dim3(1), dim3(1), 0, s, step, N);
  return (int)hipGetLastError();
}
