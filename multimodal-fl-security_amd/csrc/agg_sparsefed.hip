// SparseFed (Panda, Mahloujifar, Bhagoji, Chakraborty, Mittal, "SparseFed:
// Mitigating Model Poisoning Attacks in Federated Learning with Sparsification",
// AISTATS 2022, Algorithm 1) on gfx950: the clients' updates are clipped to a
// norm L and averaged, the average is added to a server-side error memory W, and
// only the k largest-magnitude coordinates of W are applied to the model; the
// rest stay in W for later rounds.  The attacker's reach is bounded by the
// clipping and by having to win the top-k against the honest majority's
// accumulated direction.
//
// The arithmetic is fixed (flr.h).  The calls, each enqueued on the stream with no
// host synchronisation and no allocation:
//   flr_row_norms             e_i = ||x_i - g|| (agg_norm.hip)
//   flr_sparsefed_weights     one workgroup: L, beta_i = min(1, L / e_i) / n
//   flr_sparsefed_accumulate  the K x P pass: W += [rho * U +] sum_i beta_i (x_i - g),
//                             and the level-1 histogram of W's keys on the way
//   flr_topk_abs_select       the exact magnitude top-k of any fp32 vector: a
//                             three-digit radix select on the 31-bit key, then the
//                             ties' per-chunk counts and their exclusive scan
//   flr_sparsefed_apply       out = g + W on the selected coordinates (W, U <- 0
//                             there), g elsewhere
//   flr_topk_abs_mask         the selection alone, as a byte mask
//
// The select.  key(v) = the magnitude bits, 0 for a NaN or an inf.  Digits d1 =
// key >> 20 (2048 bins), d2 = (key >> 9) & 0x7ff (2048), d3 = key & 0x1ff (512).
// Per level one histogram pass (a private LDS histogram per workgroup, flushed
// with one integer atomicAdd per non-empty bin: integer counts do not depend on
// the arrival order) and one one-workgroup scan from the top bin down.  Ties at
// the threshold go to the lowest indices: a count pass gives each chunk's
// number of keys == T, one workgroup scans the chunks, and the apply / mask pass
// adds the in-chunk rank (wave ballot prefix, the waves' counts through LDS).
// No kernel waits on another workgroup: every dependency is a kernel boundary.
//
// The chunk map.  A chunk is CHUNK = 1024 adjacent coordinates, lane t of the
// workgroup owning the four from 4 t on (one 16-byte access when the pointers
// are 16-byte aligned and all four lie inside P, else up to four 4-byte
// accesses: the same bits).  Workgroup b owns the chunks [b * per, (b + 1) * per),
// per and the grid functions of P alone (at most grid_for's 4096 workgroups).
// The accumulate pass has no order to keep and runs on rows_pass.h's lane map.
#include "rows_pass.h"

#include <cmath>

namespace flr {
namespace sparsefed {

using namespace rows;  // THREADS, the lane map, load / store, uniform, block_reduce, finite64, sort_key, rank_below
constexpr int MAXROWS = 4096;  // beta in LDS; flr_rows_combine_from's limit
constexpr int WAVES = THREADS / 64;
constexpr int CHUNK = THREADS * 4;
constexpr int BINS = 2048;  // the widest level
constexpr int BINS3 = 512;
constexpr int W_THREADS = 1024;  // the weights workgroup
constexpr int S_THREADS = 256;   // the bin scan's workgroup
constexpr int C_THREADS = 1024;  // the chunk scan's workgroup

// ---- the workspace ----
// [hist1 2048][hist2 2048][hist3 512] uint32, [state 64] uint32 (prefix, remaining
// k, n_gt), then one uint32 per chunk: the ties' counts, after the scan their
// exclusive prefix.
constexpr size_t HIST_WORDS = BINS + BINS + BINS3;
constexpr size_t STATE_WORDS = 64;
constexpr size_t HEAD_BYTES = (HIST_WORDS + STATE_WORDS) * sizeof(uint32_t);

struct ChunkMap {
  int64_t nchunks, per;
  int grid;
  explicit ChunkMap(int64_t P) {
    nchunks = (P + CHUNK - 1) / CHUNK;
    const int cap = grid_for(nchunks * THREADS);
    per = (nchunks + cap - 1) / cap;
    grid = (int)((nchunks + per - 1) / per);
  }
};

struct Workspace {
  uint32_t *hist1, *hist2, *hist3, *state, *chunks;
  explicit Workspace(void* ws) {
    hist1 = static_cast<uint32_t*>(ws);
    hist2 = hist1 + BINS;
    hist3 = hist2 + BINS;
    state = hist3 + BINS3;
    chunks = state + STATE_WORDS;
  }
};

inline size_t workspace_bytes(int64_t P) {
  return align_up(HEAD_BYTES + (size_t)ChunkMap(P).nchunks * sizeof(uint32_t), 256);
}
inline bool workspace_ok(const void* ws, size_t bytes, int64_t P) {
  return ws && bytes >= workspace_bytes(P) && (reinterpret_cast<uintptr_t>(ws) & 255) == 0;
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// ---- the key ----

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// The magnitude as an ordered integer; a NaN or an inf ranks with zero.
__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t u = __float_as_uint(x) & 0x7fffffffu;
  return u < 0x7f800000u ? u : 0u;
}

// The workgroup's LDS histogram -> the global one: one atomicAdd per non-empty bin.
template <int NB>
__device__ __forceinline__ void flush_bins(const uint32_t* lh, uint32_t* __restrict__ hist) {
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += THREADS) {
    const uint32_t n = lh[b];
    if (n != 0) atomicAdd(hist + b, n);
  }
}

// ---- flr_sparsefed_weights ----

__global__ __launch_bounds__(W_THREADS) void weights_kernel(const double* __restrict__ norms, int K, double clip,
                                                            float* __restrict__ beta, double* __restrict__ stats,
                                                            int32_t* __restrict__ flags) {
  __shared__ uint64_t keys[MAXROWS];  // a bad row's key is the largest: it ranks after every good row
  __shared__ int red[W_THREADS / 64];
  __shared__ double median;
  const int t = threadIdx.x;
  int cnt = 0;
  for (int i = t; i < K; i += W_THREADS) {
    const double e = norms[i];
    const bool good = finite64(e);
    keys[i] = good ? sort_key(e) : 0xffffffffffffffffull;
    cnt += good ? 1 : 0;
  }
  const int n = block_reduce<W_THREADS / 64>(cnt, red, [](int a, int b) { return a + b; });
  double L = 0.0;
  if (n > 0) {
    if (clip > 0.0) {
      L = clip;
    } else {
      for (int i = t; i < K; i += W_THREADS)
        if (finite64(norms[i]) && rank_below(keys, K, i) == (n - 1) / 2) median = norms[i];
      __syncthreads();
      L = median;
    }
  }
  int nclip = 0;
  for (int i = t; i < K; i += W_THREADS) {
    const double e = norms[i];
    float b = 0.f;
    if (n > 0 && finite64(e)) {
      const bool over = e > L;
      const double gamma = over ? L / e : 1.0;
      b = (float)(gamma / (double)n);
      nclip += over ? 1 : 0;
    }
    beta[i] = b;
  }
  const int clipped = block_reduce<W_THREADS / 64>(nclip, red, [](int a, int b) { return a + b; });
  if (t == 0) {
    if (stats) {
      stats[0] = L;
      stats[1] = (double)n;
      stats[2] = (double)clipped;
    }
    if (flags) *flags = (n > 0 ? 0 : 1) | (n < K ? 2 : 0);
  }
}

// ---- flr_sparsefed_accumulate ----

// W adjacent coordinates from p on: flr_rows_combine_from's accumulator (the rows
// in groups of STREAM loads, each under its wave-uniform test of beta) without
// the final + c, then the momentum, the memory and the key's level-1 bin.
// Returns the coordinates dropped.
template <int W>
__device__ __forceinline__ int accumulate_columns(const float* __restrict__ X, int K, int64_t ldx, int64_t p,
                                                  const float* __restrict__ g, const float* bs, float rho,
                                                  float* __restrict__ Wm, float* __restrict__ U, uint32_t* lh) {
  float c[W], acc[W];
  load<W>(g + p, c);
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.f;
  const float* col = X + p;
  for (int k0 = 0; k0 < K; k0 += STREAM) {
    float t[STREAM][W];
#pragma unroll
    for (int i = 0; i < STREAM; ++i) {
#pragma unroll
      for (int e = 0; e < W; ++e) t[i][e] = 0.f;
      if (k0 + i < K && uniform(bs[min(k0 + i, K - 1)]) != 0.f) load<W>(col + (int64_t)(k0 + i) * ldx, t[i]);
    }
#pragma unroll
    for (int i = 0; i < STREAM; ++i) {
      if (k0 + i < K) {
        const float bi = uniform(bs[min(k0 + i, K - 1)]);
        if (bi != 0.f) {
#pragma unroll
          for (int e = 0; e < W; ++e) acc[e] = add_rn(acc[e], mul_rn(sub_rn(t[i][e], c[e]), bi));
        }
      }
    }
  }
  float w[W], u[W];
  load<W>(Wm + p, w);
  if (U) load<W>(U + p, u);
  int ndrop = 0;
#pragma unroll
  for (int e = 0; e < W; ++e) {
    u[e] = U ? add_rn(mul_rn(rho, u[e]), acc[e]) : acc[e];
    w[e] = add_rn(w[e], u[e]);
    if (!finite32(w[e])) {
      w[e] = 0.f;
      u[e] = 0.f;
      ++ndrop;
    }
    if (lh) atomicAdd(lh + (key_of(w[e]) >> 20), 1u);
  }
  store<W>(Wm + p, w);
  if (U) store<W>(U + p, u);
  return ndrop;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void accumulate_kernel(const float* __restrict__ X, int K, int64_t P, int64_t ldx,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ beta, float rho,
                                                             float* __restrict__ Wm, float* __restrict__ U,
                                                             uint32_t* __restrict__ hist,
                                                             unsigned long long* __restrict__ dropped) {
  __shared__ float bs[MAXROWS];
  __shared__ uint32_t lh[BINS];
  __shared__ int red[WAVES];
  for (int i = threadIdx.x; i < K; i += THREADS) bs[i] = beta[i];
  for (int b = threadIdx.x; b < BINS; b += THREADS) lh[b] = 0u;
  __syncthreads();
  uint32_t* const bins = hist ? lh : nullptr;
  int ndrop = 0;
  const int64_t lanes = VEC ? P / 4 + (P & 3) : P, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < lanes; q += stride)
    lane_columns<VEC>(q, P, [&](auto w, int64_t p) {
      ndrop += accumulate_columns<decltype(w)::value>(X, K, ldx, p, g, bs, rho, Wm, U, bins);
    });
  const int total = block_reduce<WAVES>(ndrop, red, [](int a, int b) { return a + b; });
  if (dropped && threadIdx.x == 0 && total != 0) atomicAdd(dropped, (unsigned long long)total);
  if (hist) flush_bins<BINS>(lh, hist);
}

// ---- the chunk walk ----

// Lane t's four coordinates of chunk c; returns how many lie inside P (they are
// the first ones), the others read as +0.
template <bool VEC>
__device__ __forceinline__ int load_lane(const float* __restrict__ v, int64_t P, int64_t p, float (&x)[4]) {
  if (VEC && p + 4 <= P) {
    load<4>(v + p, x);
    return 4;
  }
  int n = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x[e] = 0.f;
    if (p + e < P) {
      x[e] = v[p + e];
      n = e + 1;
    }
  }
  return n;
}

// Level LEVEL's histogram of the keys that match the digits found so far
// (state[0], written by the scan of the level before).
template <bool VEC, int LEVEL>
__global__ __launch_bounds__(THREADS) void hist_kernel(const float* __restrict__ v, int64_t P, int64_t per,
                                                       int64_t nchunks, const uint32_t* __restrict__ state,
                                                       uint32_t* __restrict__ hist) {
  constexpr int NB = LEVEL == 3 ? BINS3 : BINS;
  __shared__ uint32_t lh[NB];
  for (int b = threadIdx.x; b < NB; b += THREADS) lh[b] = 0u;
  __syncthreads();
  const uint32_t prefix = LEVEL > 1 ? state[0] : 0u;
  const int64_t c1 = min64(nchunks, ((int64_t)blockIdx.x + 1) * per);
  for (int64_t c = (int64_t)blockIdx.x * per; c < c1; ++c) {
    float x[4];
    const int n = load_lane<VEC>(v, P, c * CHUNK + 4 * (int64_t)threadIdx.x, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e >= n) continue;
      const uint32_t key = key_of(x[e]);
      if constexpr (LEVEL == 1) {
        atomicAdd(lh + (key >> 20), 1u);
      } else if constexpr (LEVEL == 2) {
        if ((key >> 20) == (prefix >> 20)) atomicAdd(lh + ((key >> 9) & 0x7ffu), 1u);
      } else {
        if ((key >> 9) == (prefix >> 9)) atomicAdd(lh + (key & 0x1ffu), 1u);
      }
    }
  }
  flush_bins<NB>(lh, hist);
}

// One workgroup: from the top bin down, the bin in which the running count
// reaches the remaining k.  state: the digits so far, the remaining k, n_gt.
// Level 3 writes sel = (T, n_gt, r, 0).
__global__ __launch_bounds__(S_THREADS) void scan_kernel(const uint32_t* __restrict__ hist, int nbins, int shift,
                                                         int level, uint32_t k, uint32_t* state,
                                                         uint32_t* __restrict__ sel) {
  __shared__ uint32_t sums[S_THREADS];
  const int t = threadIdx.x, per = nbins / S_THREADS;  // 8 or 2
  uint32_t h[BINS / S_THREADS], sum = 0;
#pragma unroll
  for (int j = 0; j < BINS / S_THREADS; ++j) {
    h[j] = j < per ? hist[t * per + j] : 0u;
    sum += h[j];
  }
  const uint32_t prefix = level == 1 ? 0u : state[0];
  const uint32_t krem = level == 1 ? k : state[1];
  const uint32_t ngt = level == 1 ? 0u : state[2];
  sums[t] = sum;
  __syncthreads();  // every lane has read state before one writes it
  uint32_t running = 0;
  for (int j = t + 1; j < S_THREADS; ++j) running += sums[j];
#pragma unroll
  for (int j = BINS / S_THREADS - 1; j >= 0; --j) {
    if (j >= per) continue;
    if (running < krem && running + h[j] >= krem) {  // exactly one lane, one bin: the counts sum to >= krem
      const uint32_t found = prefix | ((uint32_t)(t * per + j) << shift);
      state[0] = found;
      state[1] = krem - running;
      state[2] = ngt + running;
      if (level == 3) {
        sel[0] = found;
        sel[1] = ngt + running;
        sel[2] = krem - running;
        sel[3] = 0u;
      }
    }
    running += h[j];
  }
}

// Each chunk's number of keys == T; a NaN or an inf anywhere sets bit 0 of *flags.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void count_kernel(const float* __restrict__ v, int64_t P, int64_t per,
                                                        int64_t nchunks, const uint32_t* sel,
                                                        uint32_t* __restrict__ cnt, uint32_t* flags) {
  __shared__ int red[WAVES];
  const uint32_t T = sel[0];
  int bad = 0;
  const int64_t c1 = min64(nchunks, ((int64_t)blockIdx.x + 1) * per);
  for (int64_t c = (int64_t)blockIdx.x * per; c < c1; ++c) {
    float x[4];
    const int n = load_lane<VEC>(v, P, c * CHUNK + 4 * (int64_t)threadIdx.x, x);
    int ties = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e >= n) continue;
      ties += key_of(x[e]) == T ? 1 : 0;
      bad |= finite32(x[e]) ? 0 : 1;
    }
    const int total = block_reduce<WAVES>(ties, red, [](int a, int b) { return a + b; });
    if (threadIdx.x == 0) cnt[c] = (uint32_t)total;
  }
  const int anybad = block_reduce<WAVES>(bad, red, [](int a, int b) { return a | b; });
  if (threadIdx.x == 0 && anybad) atomicOr(flags, 1u);
}

// One workgroup: the chunks' counts -> their exclusive prefix, in place.  A lane
// owns a contiguous segment of the chunks.
__global__ __launch_bounds__(C_THREADS) void chunk_scan_kernel(uint32_t* cnt, int64_t nchunks) {
  __shared__ uint32_t sums[C_THREADS];
  const int t = threadIdx.x;
  const int64_t seg = (nchunks + C_THREADS - 1) / C_THREADS;
  const int64_t lo = min64(nchunks, t * seg), hi = min64(nchunks, lo + seg);
  uint32_t sum = 0;
  for (int64_t c = lo; c < hi; ++c) sum += cnt[c];
  sums[t] = sum;
  __syncthreads();
  uint32_t base = 0;
  for (int j = 0; j < t; ++j) base += sums[j];
  for (int64_t c = lo; c < hi; ++c) {
    const uint32_t n = cnt[c];
    cnt[c] = base;
    base += n;
  }
}

// Lane t's four coordinates of chunk c and which of them are selected: key > T,
// or key == T with fewer than r ties at lower indices (base: the ties in the
// chunks before).  wcnt: WAVES entries of LDS.  Every lane of the workgroup calls it.
template <bool VEC>
__device__ __forceinline__ int select_lane(const float* __restrict__ v, int64_t P, int64_t p, uint32_t T, uint32_t r,
                                           uint32_t base, uint32_t* wcnt, float (&x)[4], bool (&s)[4]) {
  const int n = load_lane<VEC>(v, P, p, x);
  bool tie[4], gt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t before = 0, wave_total = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t key = key_of(x[e]);
    tie[e] = e < n && key == T;
    gt[e] = e < n && key > T;
    const unsigned long long b = __ballot(tie[e]);
    before += (uint32_t)__popcll(b & below);
    wave_total += (uint32_t)__popcll(b);
  }
  __syncthreads();  // the chunk before has read wcnt
  if (lane == 0) wcnt[wave] = wave_total;
  __syncthreads();
  for (int w = 0; w < wave; ++w) before += wcnt[w];
  uint32_t rank = base + before;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s[e] = gt[e] || (tie[e] && rank < r);
    rank += tie[e] ? 1u : 0u;
  }
  return n;
}

// The lane's n mask bytes from p on: one 4-byte store when the mask is 4-byte aligned.
__device__ __forceinline__ void store_mask(uint8_t* __restrict__ mask, bool word, int64_t p, int n,
                                           const bool (&s)[4]) {
  if (word && n == 4) {
    *reinterpret_cast<uint32_t*>(mask + p) =
        (s[0] ? 1u : 0u) | (s[1] ? 0x100u : 0u) | (s[2] ? 0x10000u : 0u) | (s[3] ? 0x1000000u : 0u);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) mask[p + e] = s[e] ? 1 : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void mask_kernel(const float* __restrict__ v, int64_t P, int64_t per,
                                                       int64_t nchunks, const uint32_t* __restrict__ sel,
                                                       const uint32_t* __restrict__ off, uint8_t* __restrict__ mask,
                                                       bool word) {
  __shared__ uint32_t wcnt[WAVES];
  const uint32_t T = sel[0], r = sel[2];
  const int64_t c1 = min64(nchunks, ((int64_t)blockIdx.x + 1) * per);
  for (int64_t c = (int64_t)blockIdx.x * per; c < c1; ++c) {
    const int64_t p = c * CHUNK + 4 * (int64_t)threadIdx.x;
    float x[4];
    bool s[4];
    const int n = select_lane<VEC>(v, P, p, T, r, off[c], wcnt, x, s);
    store_mask(mask, word, p, n, s);
  }
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void apply_kernel(const float* __restrict__ g, float* __restrict__ Wm,
                                                        float* __restrict__ U, int64_t P, int64_t per, int64_t nchunks,
                                                        const uint32_t* __restrict__ sel,
                                                        const uint32_t* __restrict__ off, float* __restrict__ out,
                                                        uint8_t* __restrict__ mask, bool word) {
  __shared__ uint32_t wcnt[WAVES];
  const uint32_t T = sel[0], r = sel[2];
  const int64_t c1 = min64(nchunks, ((int64_t)blockIdx.x + 1) * per);
  for (int64_t c = (int64_t)blockIdx.x * per; c < c1; ++c) {
    const int64_t p = c * CHUNK + 4 * (int64_t)threadIdx.x;
    float w[4];
    bool s[4];
    const int n = select_lane<VEC>(Wm, P, p, T, r, off[c], wcnt, w, s);
    if (VEC && n == 4) {
      float c4[4], o[4];
      load<4>(g + p, c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = s[e] ? add_rn(c4[e], w[e]) : c4[e];
        w[e] = s[e] ? 0.f : w[e];
      }
      store<4>(out + p, o);
      if (s[0] || s[1] || s[2] || s[3]) {
        store<4>(Wm + p, w);
        if (U) {
          float u[4];
          load<4>(U + p, u);
#pragma unroll
          for (int e = 0; e < 4; ++e) u[e] = s[e] ? 0.f : u[e];
          store<4>(U + p, u);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e >= n) continue;
        const float gv = g[p + e];
        out[p + e] = s[e] ? add_rn(gv, w[e]) : gv;
        if (s[e]) {
          Wm[p + e] = 0.f;
          if (U) U[p + e] = 0.f;
        }
      }
    }
    if (mask) store_mask(mask, word, p, n, s);
  }
}

inline int zero_bytes(void* p, size_t bytes, hipStream_t st, const char* where) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
  if (e != hipSuccess) {
    set_last_error(where, e);
    return FLR_ERR_HIP;
  }
  return FLR_OK;
}

template <int LEVEL>
inline int launch_hist(bool vec, const ChunkMap& cm, const float* v, int64_t P, const uint32_t* state, uint32_t* hist,
                       hipStream_t st) {
  const dim3 grid((unsigned)cm.grid), block(THREADS);
  if (vec)
    hipLaunchKernelGGL((hist_kernel<true, LEVEL>), grid, block, 0, st, v, P, cm.per, cm.nchunks, state, hist);
  else
    hipLaunchKernelGGL((hist_kernel<false, LEVEL>), grid, block, 0, st, v, P, cm.per, cm.nchunks, state, hist);
  return launch_status("topk_abs histogram");
}

inline int launch_scan(const uint32_t* hist, int nbins, int shift, int level, uint32_t k, uint32_t* state,
                       uint32_t* sel, hipStream_t st) {
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(S_THREADS), 0, st, hist, nbins, shift, level, k, state, sel);
  return launch_status("topk_abs scan");
}

}  // namespace sparsefed
}  // namespace flr

using namespace flr;

extern "C" int flr_sparsefed_weights(const double* norms, int64_t K, double clip_norm, float* beta, double* stats,
                                     int32_t* flags, void* stream) {
  if (!norms || !beta || K < 1 || !(clip_norm >= 0.0) || !(clip_norm < __builtin_huge_val())) return FLR_ERR_ARG;
  if (K > sparsefed::MAXROWS) return FLR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sparsefed::weights_kernel, dim3(1), dim3(sparsefed::W_THREADS), 0, as_stream(stream), norms,
                     (int)K, clip_norm, beta, stats, flags);
  return launch_status("sparsefed_weights");
}

extern "C" int flr_sparsefed_accumulate(const float* X, int64_t K, int64_t P, int64_t ldx, const float* g,
                                        const float* beta, float rho, float* W, float* U, uint32_t* hist,
                                        int64_t* dropped, void* stream) {
  if (!X || !g || !beta || !W || K < 1 || P < 0 || ldx < P || !(rho >= 0.f) || !(rho < 1.f) || (rho != 0.f && !U) ||
      W == g || (U && (U == W || U == g)))
    return FLR_ERR_ARG;
  if (K > sparsefed::MAXROWS || P >= (int64_t)1 << 32) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  hipStream_t st = as_stream(stream);
  int rc = FLR_OK;
  if (hist) rc = sparsefed::zero_bytes(hist, sparsefed::BINS * sizeof(uint32_t), st, "sparsefed histogram memset");
  if (rc == FLR_OK && dropped) rc = sparsefed::zero_bytes(dropped, sizeof(int64_t), st, "sparsefed dropped memset");
  if (rc != FLR_OK) return rc;
  float* Um = rho != 0.f ? U : nullptr;  // rho == 0: U is not touched
  const bool vec = rows::vec_ok(X, g, W, Um, ldx);
  const dim3 grid(rows::grid_for(rows::column_lanes(vec, P))), block(sparsefed::THREADS);
  unsigned long long* dr = reinterpret_cast<unsigned long long*>(dropped);
  if (vec)
    hipLaunchKernelGGL(sparsefed::accumulate_kernel<true>, grid, block, 0, st, X, (int)K, P, ldx, g, beta, rho, W, Um,
                       hist, dr);
  else
    hipLaunchKernelGGL(sparsefed::accumulate_kernel<false>, grid, block, 0, st, X, (int)K, P, ldx, g, beta, rho, W, Um,
                       hist, dr);
  return launch_status("sparsefed_accumulate");
}

extern "C" size_t flr_topk_abs_workspace(int64_t P) {
  return (P < 1 || P >= (int64_t)1 << 32) ? 0 : sparsefed::workspace_bytes(P);
}

extern "C" int flr_topk_abs_select(const float* v, int64_t P, int64_t k, const uint32_t* hist1, uint32_t* sel,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!v || !sel || P < 0) return FLR_ERR_ARG;
  if (P >= (int64_t)1 << 32) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  if (k < 1 || k > P) return FLR_ERR_ARG;
  if (!sparsefed::workspace_ok(workspace, workspace_bytes, P)) return FLR_ERR_WORKSPACE;
  const sparsefed::Workspace ws(workspace);
  const sparsefed::ChunkMap cm(P);
  hipStream_t st = as_stream(stream);
  int rc = sparsefed::zero_bytes(workspace, sparsefed::HEAD_BYTES, st, "topk_abs workspace memset");
  if (rc != FLR_OK) return rc;
  const bool vec = rows::vec_ok(v);
  const uint32_t kk = (uint32_t)k;
  if (!hist1) {
    if ((rc = sparsefed::launch_hist<1>(vec, cm, v, P, ws.state, ws.hist1, st)) != FLR_OK) return rc;
    hist1 = ws.hist1;
  }
  if ((rc = sparsefed::launch_scan(hist1, sparsefed::BINS, 20, 1, kk, ws.state, sel, st)) != FLR_OK) return rc;
  if ((rc = sparsefed::launch_hist<2>(vec, cm, v, P, ws.state, ws.hist2, st)) != FLR_OK) return rc;
  if ((rc = sparsefed::launch_scan(ws.hist2, sparsefed::BINS, 9, 2, kk, ws.state, sel, st)) != FLR_OK) return rc;
  if ((rc = sparsefed::launch_hist<3>(vec, cm, v, P, ws.state, ws.hist3, st)) != FLR_OK) return rc;
  if ((rc = sparsefed::launch_scan(ws.hist3, sparsefed::BINS3, 0, 3, kk, ws.state, sel, st)) != FLR_OK) return rc;
  const dim3 grid((unsigned)cm.grid), block(sparsefed::THREADS);
  if (vec)
    hipLaunchKernelGGL(sparsefed::count_kernel<true>, grid, block, 0, st, v, P, cm.per, cm.nchunks, sel, ws.chunks,
                       sel + 3);
  else
    hipLaunchKernelGGL(sparsefed::count_kernel<false>, grid, block, 0, st, v, P, cm.per, cm.nchunks, sel, ws.chunks,
                       sel + 3);
  if ((rc = launch_status("topk_abs count")) != FLR_OK) return rc;
  hipLaunchKernelGGL(sparsefed::chunk_scan_kernel, dim3(1), dim3(sparsefed::C_THREADS), 0, st, ws.chunks, cm.nchunks);
  return launch_status("topk_abs chunk scan");
}

extern "C" int flr_topk_abs_mask(const float* v, int64_t P, const uint32_t* sel, const void* workspace,
                                 size_t workspace_bytes, uint8_t* mask, void* stream) {
  if (!v || !sel || !mask || P < 0) return FLR_ERR_ARG;
  if (P >= (int64_t)1 << 32) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  if (!sparsefed::workspace_ok(workspace, workspace_bytes, P)) return FLR_ERR_WORKSPACE;
  const sparsefed::Workspace ws(const_cast<void*>(workspace));
  const sparsefed::ChunkMap cm(P);
  const bool word = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const dim3 grid((unsigned)cm.grid), block(sparsefed::THREADS);
  hipStream_t st = as_stream(stream);
  if (rows::vec_ok(v))
    hipLaunchKernelGGL(sparsefed::mask_kernel<true>, grid, block, 0, st, v, P, cm.per, cm.nchunks, sel, ws.chunks,
                       mask, word);
  else
    hipLaunchKernelGGL(sparsefed::mask_kernel<false>, grid, block, 0, st, v, P, cm.per, cm.nchunks, sel, ws.chunks,
                       mask, word);
  return launch_status("topk_abs_mask");
}

extern "C" int flr_sparsefed_apply(const float* g, float* W, float* U, int64_t P, const uint32_t* sel,
                                   const void* workspace, size_t workspace_bytes, float* out, uint8_t* mask,
                                   void* stream) {
  if (!g || !W || !sel || !out || P < 0 || out == g || out == W || W == g || (U && (U == W || U == g || U == out)))
    return FLR_ERR_ARG;
  if (P >= (int64_t)1 << 32) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  if (!sparsefed::workspace_ok(workspace, workspace_bytes, P)) return FLR_ERR_WORKSPACE;
  const sparsefed::Workspace ws(const_cast<void*>(workspace));
  const sparsefed::ChunkMap cm(P);
  const bool word = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const dim3 grid((unsigned)cm.grid), block(sparsefed::THREADS);
  hipStream_t st = as_stream(stream);
  if (rows::vec_ok(g, W, U, out))
    hipLaunchKernelGGL(sparsefed::apply_kernel<true>, grid, block, 0, st, g, W, U, P, cm.per, cm.nchunks, sel,
                       ws.chunks, out, mask, word);
  else
    hipLaunchKernelGGL(sparsefed::apply_kernel<false>, grid, block, 0, st, g, W, U, P, cm.per, cm.nchunks, sel,
                       ws.chunks, out, mask, word);
  return launch_status("sparsefed_apply");
}
