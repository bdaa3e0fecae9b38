// a11 / a14 — row-subset mean (Multi-Krum) and example-weighted FedAvg.
//
// Both are one pass over the client matrix: HBM-bound, 16-B loads per lane.
// Summation order and rounding restate the reference exactly:
//   Multi-Krum (src/defenses/krum.py:186-190):
//     param_sum = sum(u[param_idx] for u in selected_updates)  # 0 + u0 + u1 ...
//     param_sum / multi_k                                     # IEEE fp32 div
//   FedAvg (src/defenses/base_defense.py:90-95, run_experiments.py:246-254):
//     sum(n_i * u_i for i in clients) / total                 # fp32 mul, add, div
// Python's sum() starts from int 0, so the first add is 0 + u0 (turns -0 into
// +0); that is kept.  Every op is a separately rounded fp32 op (no FMA).
//
// flr_rows_mean_keep (DnC's aggregate, agg_dnc.hip) is the same mean over the rows
// with keep != 0: their ascending list is compacted into LDS by one wave (ballot +
// popcount), then the sum with 16 loads in flight per lane — only kept rows are
// read.
//
// The grid-stride loop, its scalar tail and the sum itself are rows_pass.h's
// column_sum; each kernel here is its LDS set-up and one call.
#include "rows_pass.h"

#include <algorithm>

namespace flr {
namespace mean {

using namespace rows;  // THREADS, grid_for, vec_ok, column_sum, stream_rows (rows_pass.h)
constexpr int MAXROWS = 4096;

template <bool VEC>
__global__ __launch_bounds__(THREADS) void rows_mean_kernel(const float* __restrict__ X, int64_t P,
                                                            int64_t ldx, const int32_t* __restrict__ rows,
                                                            int m, float fm, float* __restrict__ out,
                                                            uint32_t rmax) {
  __shared__ int32_t rs[MAXROWS];
  // an index outside [0, K) is clamped into range: no out-of-bounds read (flr.h)
  for (int t = threadIdx.x; t < m; t += THREADS) rs[t] = (int32_t)min((uint32_t)rows[t], rmax);
  __syncthreads();
  column_sum<VEC>(X, P, ldx, m, [&](int t) { return rs[t]; }, [](int, float x) { return x; }, fm, out);
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void fedavg_kernel(const float* __restrict__ X, int K, int64_t P,
                                                         int64_t ldx, const int64_t* __restrict__ n,
                                                         float* __restrict__ out) {
  __shared__ float wts[MAXROWS];
  __shared__ float total_f;
  for (int i = threadIdx.x; i < K; i += THREADS) wts[i] = (float)n[i];
  if (threadIdx.x == 0) {
    int64_t tot = 0;
    for (int i = 0; i < K; ++i) tot += n[i];
    total_f = (float)tot;
  }
  __syncthreads();
  column_sum<VEC>(X, P, ldx, K, [](int i) { return i; }, [&](int i, float x) { return mul_rn(wts[i], x); }, total_f,
                  out);
}

// rows_mean over a matrix whose dead-tap ranges are not written (the round
// engine's FLR_DEFER_DEAD=2): float4 groups wholly inside a dead range are
// skipped (their rows are never read), then dead_mean_kernel writes those
// coordinates from the global vector — row k's value there is gdead (negated
// for k < nneg), summed in the same order as rows_mean_kernel's: bit-identical
// to the mean of the filled rows.
constexpr int MAXDEAD = 96;
struct DeadRanges {
  int64_t off[MAXDEAD], end[MAXDEAD];
  int n;
};
__global__ __launch_bounds__(THREADS) void rows_mean_live_kernel(const float* __restrict__ X, int64_t P, int64_t ldx,
                                                                 const int32_t* __restrict__ rows, int m, float fm,
                                                                 float* __restrict__ out, uint32_t rmax,
                                                                 const DeadRanges dr) {
  __shared__ int32_t rs[MAXROWS];
  for (int t = threadIdx.x; t < m; t += THREADS) rs[t] = (int32_t)min((uint32_t)rows[t], rmax);
  __syncthreads();
  // a dead scalar tail is summed all the same and rewritten by dead_mean_kernel
  column_sum<true>(X, P, ldx, m, [&](int t) { return rs[t]; }, [](int, float x) { return x; }, fm, out,
                   [&](int64_t p) {
                     bool skip = false;
                     for (int r = 0; r < dr.n; ++r) skip |= p >= dr.off[r] && p + 4 <= dr.end[r];
                     return skip;
                   });
}
// grid (slices, ranges): out[p] of dead range r from gdead[p] and the rows' signs
__global__ __launch_bounds__(THREADS) void dead_mean_kernel(const float* __restrict__ g,
                                                            const int32_t* __restrict__ rows, int m, float fm,
                                                            uint32_t rmax, int nneg, float* __restrict__ out,
                                                            const DeadRanges dr) {
  __shared__ float sg[MAXROWS];
  for (int t = threadIdx.x; t < m; t += THREADS) sg[t] = (int)min((uint32_t)rows[t], rmax) < nneg ? -1.f : 1.f;
  __syncthreads();
  const int r = blockIdx.y;
  for (int64_t p = dr.off[r] + (int64_t)blockIdx.x * THREADS + threadIdx.x; p < dr.end[r];
       p += (int64_t)gridDim.x * THREADS) {
    const float gv = g[p];
    float acc = 0.f;
    for (int t = 0; t < m; ++t) acc = add_rn(acc, gv * sg[t]);  // the row's value: exactly +-gv
    out[p] = div_rn(acc, fm);
  }
}

// W adjacent coordinates from p on: the m listed rows streamed (stream_rows), a
// row index one wave-uniform value.  m == 0: 0 / 0.
template <int W>
__device__ __forceinline__ void mean_columns(const float* __restrict__ X, int64_t ldx, int64_t p, const int32_t* rs,
                                             int m, float fm, float* __restrict__ out) {
  float acc[W];
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.f;
  stream_rows<W>(X + p, ldx, m, [&](int t) { return __builtin_amdgcn_readfirstlane(rs[t]); },
                 [&](int, const float(&x)[W]) {
#pragma unroll
                   for (int e = 0; e < W; ++e) acc[e] = add_rn(acc[e], x[e]);
                 });
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = div_rn(acc[e], fm);
  store<W>(out + p, acc);
}

// The mean of the rows with keep != 0.  Wave 0 compacts their indices, ascending,
// into LDS (ballot + popcount per 64 rows): the row loop reads kept rows only, a
// wave-uniform index per load.  The lanes stride over the lane map (lane_columns).
// Streamed, where rows_mean_kernel's loop is plain: at a small m the stream
// re-reads the last row up to 15 times, so the two are not one kernel.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void rows_mean_keep_kernel(const float* __restrict__ X, int K, int64_t P,
                                                                 int64_t ldx, const int32_t* __restrict__ keep,
                                                                 float* __restrict__ out) {
  __shared__ int32_t rs[MAXROWS];
  __shared__ int m_s;
  if (threadIdx.x < 64) {
    int base = 0;
    for (int i0 = 0; i0 < K; i0 += 64) {
      const int i = i0 + (int)threadIdx.x;
      const bool k = i < K && keep[i] != 0;
      const unsigned long long mask = __ballot(k);
      if (k) rs[base + __popcll(mask & ((1ull << threadIdx.x) - 1ull))] = i;
      base += __popcll(mask);
    }
    if (threadIdx.x == 0) m_s = base;
  }
  __syncthreads();
  const int m = m_s;
  const float fm = (float)m;
  const int64_t lanes = VEC ? P / 4 + (P & 3) : P, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < lanes; q += stride)
    lane_columns<VEC>(q, P, [&](auto w, int64_t p) { mean_columns<decltype(w)::value>(X, ldx, p, rs, m, fm, out); });
}

}  // namespace mean
}  // namespace flr

using namespace flr;

extern "C" int flr_rows_mean(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* rows,
                             int64_t m, int64_t divisor, float* out, void* stream) {
  if (K < 1 || P < 0 || ldx < P || m < 1 || m > K || divisor < 1 || !X || !rows || !out) return FLR_ERR_ARG;
  const float fdiv = (float)divisor;
  if (m > mean::MAXROWS) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  hipStream_t st = as_stream(stream);
  if (mean::vec_ok(X, out, ldx)) {
    hipLaunchKernelGGL(mean::rows_mean_kernel<true>, dim3(mean::grid_for(P / 4)), dim3(mean::THREADS), 0, st,
                       X, P, ldx, rows, (int)m, fdiv, out, (uint32_t)(K - 1));
  } else {
    hipLaunchKernelGGL(mean::rows_mean_kernel<false>, dim3(mean::grid_for(P)), dim3(mean::THREADS), 0, st, X,
                       P, ldx, rows, (int)m, fdiv, out, (uint32_t)(K - 1));
  }
  return launch_status("rows_mean_kernel");
}

extern "C" int flr_rows_mean_dead(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* rows,
                                  int64_t m, int64_t divisor, const int64_t* dead_off, const int64_t* dead_n,
                                  int64_t ndead, const float* gdead, int64_t nneg, float* out, void* stream) {
  if (K < 1 || P < 0 || ldx < P || m < 1 || m > K || divisor < 1 || !X || !rows || !out || ndead < 0 || nneg < 0 ||
      (ndead > 0 && (!dead_off || !dead_n || !gdead)))
    return FLR_ERR_ARG;
  if (m > mean::MAXROWS || ndead > mean::MAXDEAD) return FLR_ERR_UNSUPPORTED;
  mean::DeadRanges dr;
  dr.n = (int)ndead;
  int64_t longest = 0;
  for (int64_t r = 0; r < ndead; ++r) {
    if (dead_off[r] < 0 || dead_n[r] < 0 || dead_off[r] + dead_n[r] > P) return FLR_ERR_ARG;
    dr.off[r] = dead_off[r];
    dr.end[r] = dead_off[r] + dead_n[r];
    longest = std::max(longest, dead_n[r]);
  }
  if (P == 0) return FLR_OK;
  if (!mean::vec_ok(X, out, ldx)) return FLR_ERR_ARG;  // the engine's matrix: 16-B rows
  hipStream_t st = as_stream(stream);
  const float fdiv = (float)divisor;
  hipLaunchKernelGGL(mean::rows_mean_live_kernel, dim3(mean::grid_for(P / 4)), dim3(mean::THREADS), 0, st, X, P, ldx,
                     rows, (int)m, fdiv, out, (uint32_t)(K - 1), dr);
  int rc = launch_status("rows_mean_live_kernel");
  if (rc != FLR_OK || ndead == 0 || longest == 0) return rc;
  const int gx = (int)std::min<int64_t>(256, (longest + mean::THREADS - 1) / mean::THREADS);
  hipLaunchKernelGGL(mean::dead_mean_kernel, dim3((unsigned)gx, (unsigned)ndead), dim3(mean::THREADS), 0, st, gdead,
                     rows, (int)m, fdiv, (uint32_t)(K - 1), (int)std::min<int64_t>(nneg, K), out, dr);
  return launch_status("dead_mean_kernel");
}

extern "C" int flr_fedavg(const float* X, int64_t K, int64_t P, int64_t ldx, const int64_t* num_examples,
                          float* out, void* stream) {
  if (K < 1 || P < 0 || ldx < P || !X || !num_examples || !out) return FLR_ERR_ARG;
  if (K > mean::MAXROWS) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  hipStream_t st = as_stream(stream);
  if (mean::vec_ok(X, out, ldx)) {
    hipLaunchKernelGGL(mean::fedavg_kernel<true>, dim3(mean::grid_for(P / 4)), dim3(mean::THREADS), 0, st, X,
                       (int)K, P, ldx, num_examples, out);
  } else {
    hipLaunchKernelGGL(mean::fedavg_kernel<false>, dim3(mean::grid_for(P)), dim3(mean::THREADS), 0, st, X,
                       (int)K, P, ldx, num_examples, out);
  }
  return launch_status("fedavg_kernel");
}

extern "C" int flr_rows_mean_keep(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* keep, float* out,
                                  void* stream) {
  if (!X || !keep || !out || K < 1 || P < 0 || ldx < P) return FLR_ERR_ARG;
  if (K > mean::MAXROWS) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  const bool vec = mean::vec_ok(X, out, ldx);
  const dim3 grid(mean::grid_for(mean::column_lanes(vec, P))), block(mean::THREADS);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(mean::rows_mean_keep_kernel<true>, grid, block, 0, st, X, (int)K, P, ldx, keep, out);
  else
    hipLaunchKernelGGL(mean::rows_mean_keep_kernel<false>, grid, block, 0, st, X, (int)K, P, ldx, keep, out);
  return launch_status("rows_mean_keep");
}
