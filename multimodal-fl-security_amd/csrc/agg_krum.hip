// a10 — Krum score + selection on the device.
//
// Replaces KrumDefense._krum_score and the selection in aggregate
// (src/defenses/krum.py:101-131, 149-176):
//   sorted = np.sort(distances[i]); score = np.sum(sorted[1 : m + 1])
//   order  = np.argsort(scores)
// np.sum over a contiguous float64 slice is numpy's pairwise summation
// (8 accumulators for n <= 128, recursive halving above); it is restated
// exactly here, so scores are bit-identical to numpy given the same D.
// np.argsort's default quicksort is not stable; exact score ties are broken
// here by the lower client index (documented divergence, tests flag ties).
// NaN as numpy orders it: np.sort and np.argsort put NaN after +inf, so a
// NaN distance lands in a row's last ranks and a NaN score (a client that sent
// NaN) is ranked last — rejected, not selected.  Every order slot is written.
#include "flr_common.h"

namespace flr {
namespace krum {

constexpr int MAXK = 1024;

// a sorts after b in numpy's order (NaN after everything, NaNs equal)
__device__ __forceinline__ bool np_after(double a, double b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool np_equal(double a, double b) { return a == b || (a != a && b != b); }

// numpy pairwise_sum_DOUBLE (numpy/_core/src/umath/loops_utils.h.src), exact.
template <int DEPTH>
__device__ double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128 || DEPTH == 0) {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  if constexpr (DEPTH > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum<DEPTH - 1>(a, n2) + np_pairwise_sum<DEPTH - 1>(a + n2, n - n2);
  }
  return 0.0;
}

// One workgroup per client row: bitonic sort of the row in LDS, then the
// numpy pairwise sum of ranks 1..m.
__global__ __launch_bounds__(256) void score_kernel(const double* __restrict__ D, int K, int m,
                                                    double* __restrict__ scores) {
  __shared__ double s[MAXK];
  const int i = blockIdx.x;
  int np2 = 1;
  while (np2 < K) np2 <<= 1;
  for (int j = threadIdx.x; j < np2; j += blockDim.x)
    s[j] = j < K ? D[(int64_t)i * K + j] : __builtin_nan("");  // pads sort with the NaNs, after every value
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = threadIdx.x; idx < np2; idx += blockDim.x) {
        const int ixj = idx ^ j;
        if (ixj > idx) {
          const double a = s[idx], b = s[ixj];
          const bool up = (idx & k) == 0;
          if ((up && np_after(a, b)) || (!up && np_after(b, a))) {
            s[idx] = b;
            s[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) scores[i] = 0.0 + np_pairwise_sum<4>(s + 1, m);
}

// Stable rank: order[rank(i)] = i.
__global__ __launch_bounds__(1024) void order_kernel(const double* __restrict__ scores, int K,
                                                     int32_t* __restrict__ order) {
  __shared__ double s[MAXK];
  for (int j = threadIdx.x; j < K; j += blockDim.x) s[j] = scores[j];
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    const double si = s[i];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const double sj = s[j];
      rank += np_after(si, sj) || (np_equal(sj, si) && j < i);
    }
    order[rank] = i;
  }
}

// ---- Bulyan's first stage: Krum re-run on the shrinking set ---------------------
// theta + 1 stream-ordered launches of one kernel, no host round trip.  Launch
// `it` first closes iteration it - 1: every workgroup rebuilds the alive set
// (every client not in picked[0, it - 1), written by earlier launches) and
// takes the argmin of that iteration's scores over it itself (K values: cheaper
// than a launch of its own), workgroup 0 records the pick.  It then scores its
// own client for iteration `it` against the clients still alive, as
// score_kernel does on the whole row: the dead columns are loaded as the NaN
// padding, which sorts after every value, and ranks 1..m of the sorted row
// hold alive entries only (m <= n_r - 1).  The scores are double-buffered by
// iteration parity: a workgroup writes iteration it's while others still read
// iteration it - 1's.  Launch theta only closes the last iteration and lists
// the unpicked clients in ascending index.
constexpr int ITER_THREADS = 256;

// (sa, ia) is picked before (sb, ib): the smaller score, an exact tie to the
// lower index, NaN last; index -1 is no candidate
__device__ __forceinline__ bool picks_before(double sa, int ia, double sb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return np_after(sb, sa) || (np_equal(sa, sb) && ia < ib);
}

__global__ __launch_bounds__(ITER_THREADS) void iter_kernel(const double* __restrict__ D, int K, int f, int it,
                                                            int theta, double* __restrict__ sc,
                                                            double* __restrict__ scores,
                                                            int32_t* __restrict__ picked) {
  __shared__ double s[MAXK];
  __shared__ unsigned char alive[MAXK];
  __shared__ double rs[ITER_THREADS];
  __shared__ int ri[ITER_THREADS];
  const int tid = threadIdx.x;
  for (int j = tid; j < K; j += ITER_THREADS) alive[j] = 1;
  __syncthreads();
  for (int j = tid; j < it - 1; j += ITER_THREADS) alive[min(max(picked[j], 0), K - 1)] = 0;
  __syncthreads();
  if (it > 0) {
    const double* prev = sc + (size_t)((it - 1) & 1) * K;
    double bs = 0.0;
    int bi = -1;
    for (int j = tid; j < K; j += ITER_THREADS) {  // ascending j: a tie keeps the lower index
      if (!alive[j]) continue;
      const double sj = prev[j];
      if (picks_before(sj, j, bs, bi)) {
        bs = sj;
        bi = j;
      }
    }
    rs[tid] = bs;
    ri[tid] = bi;
    __syncthreads();
    for (int w = ITER_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w && picks_before(rs[tid + w], ri[tid + w], rs[tid], ri[tid])) {
        rs[tid] = rs[tid + w];
        ri[tid] = ri[tid + w];
      }
      __syncthreads();
    }
    const int pick = min(max(ri[0], 0), K - 1);  // an alive client always exists (it - 1 < theta <= K)
    if (tid == 0) {
      alive[pick] = 0;
      if (blockIdx.x == 0) picked[it - 1] = pick;
    }
    __syncthreads();
  }
  if (it >= theta) {  // the closing launch: the unpicked clients, ascending
    if (blockIdx.x == 0 && tid == 0) {
      int n = theta;
      for (int j = 0; j < K; ++j)
        if (alive[j] && n < K) picked[n++] = j;
    }
    return;
  }
  const int i = blockIdx.x;
  if (!alive[i]) return;
  const int nr = K - it;
  const int m = min(nr - 1, max(1, nr - f - 2));
  int np2 = 1;
  while (np2 < K) np2 <<= 1;
  for (int j = tid; j < np2; j += ITER_THREADS)
    s[j] = (j < K && alive[j]) ? D[(int64_t)i * K + j] : __builtin_nan("");
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < np2; idx += ITER_THREADS) {
        const int ixj = idx ^ j;
        if (ixj > idx) {
          const double a = s[idx], b = s[ixj];
          const bool up = (idx & k) == 0;
          if ((up && np_after(a, b)) || (!up && np_after(b, a))) {
            s[idx] = b;
            s[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const double v = 0.0 + np_pairwise_sum<4>(s + 1, m);
    sc[(size_t)(it & 1) * K + i] = v;
    if (it == 0) scores[i] = v;
  }
}

}  // namespace krum
}  // namespace flr

using namespace flr;

extern "C" int flr_krum_select(const double* D, int64_t K, int64_t f, double* scores,
                               int32_t* order, void* stream) {
  if (K < 1 || f < 0 || !D || !scores || !order) return FLR_ERR_ARG;
  if (K < 2 * f + 3) return FLR_ERR_KRUM_N;
  if (K > krum::MAXK) return FLR_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int m = (int)(K - f - 2);
  hipLaunchKernelGGL(krum::score_kernel, dim3((int)K), dim3(256), 0, st, D, (int)K, m, scores);
  int rc = launch_status("krum score_kernel");
  if (rc != FLR_OK) return rc;
  hipLaunchKernelGGL(krum::order_kernel, dim3(1), dim3(1024), 0, st, scores, (int)K, order);
  return launch_status("krum order_kernel");
}

extern "C" size_t flr_krum_select_iter_workspace(int64_t K) {
  return K > 0 ? (size_t)K * 2 * sizeof(double) : 0;  // the scores of two successive iterations
}

extern "C" int flr_krum_select_iter(const double* D, int64_t K, int64_t f, int64_t theta, double* scores,
                                    int32_t* picked, void* workspace, size_t workspace_bytes, void* stream) {
  if (K < 1 || f < 0 || theta < 1 || theta > K || !D || !scores || !picked) return FLR_ERR_ARG;
  if (K > krum::MAXK) return FLR_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < flr_krum_select_iter_workspace(K)) return FLR_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  double* sc = static_cast<double*>(workspace);
  for (int it = 0; it <= (int)theta; ++it) {
    const int grid = it < (int)theta ? (int)K : 1;
    hipLaunchKernelGGL(krum::iter_kernel, dim3(grid), dim3(krum::ITER_THREADS), 0, st, D, (int)K, (int)f, it,
                       (int)theta, sc, scores, picked);
    const int rc = launch_status("krum iter_kernel");
    if (rc != FLR_OK) return rc;
  }
  return FLR_OK;
}
