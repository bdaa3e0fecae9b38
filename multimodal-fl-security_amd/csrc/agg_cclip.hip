// Centered clipping (Karimireddy, He, Jaggi, "Learning from History for
// Byzantine Robust Optimization", ICML 2021) on gfx950: from the previous global
// model v0, iters times
//   v <- v + (1/K) * sum_i (x_i - v) * min(1, tau / ||x_i - v||)
// Each step moves v by at most tau, whatever the clipped rows hold: the defense
// for the attacks that stay inside the benign spread (attack_colluding.hip).
//
// The arithmetic is fixed (flr.h).  Iteration l, v = v_l:
//   distances  d_i = ||x_i - v||: flr_row_norms (agg_norm.hip) — fp32 differences,
//              fp64 fixed-order sum, fp64 square root
//   scales     d32 = (float)d_i;  t = tau, or when tau == 0 the lower median
//              sort(d32)[(K-1)/2], NaN last;  s_i = 0 if d32 is NaN, t / d32 if
//              d32 > t (correctly rounded; +inf gives 0), else 1
//   step       acc = +0.f;  for i in 0..K-1: if s_i != 0: acc = acc + (x_i - v) * s_i
//              v' = v + acc / (float)K     every op a separately rounded fp32 op
// A row with s_i == 0 is skipped, never multiplied: a NaN or inf client cannot
// poison the aggregate.  A torch CPU loop over the rows gives the same bits.
//
// Engine: all iters iterations are enqueued by the one C call, no host round
// trip (as flr_krum_select_iter): per iteration the two row_norms kernels, the
// one-workgroup scales kernel and the step.  The step is HBM-bound (it reads
// K * P * 4 bytes and writes P * 4): one lane per float4 of coordinates — each
// load instruction reads 1 KiB contiguous bytes of one row — with a scalar lane
// per coordinate of the P mod 4 tail; one lane per coordinate when X, v or out is
// not 16-B aligned or ldx % 4 != 0 (rows_pass.h's lane map).  The rows are streamed
// with 16 loads in flight per lane (its stream_rows); the K scales sit in LDS and reach the lanes as one
// wave-uniform value per row, so the skip is a scalar branch.  The iterates
// alternate between out and a P-vector of the workspace, the last one in out.
#include "rows_pass.h"

namespace flr {
namespace cclip {

using namespace rows;          // THREADS, STREAM, the lane map, the row stream (rows_pass.h)
constexpr int MAXROWS = 4096;  // the scales in LDS; flr_weighted_rows' limit

// One workgroup.  t and the K scales from the K distances; tau == 0: t is the
// lower median by rank counting (each row's rank = the keys below it, equal keys
// in index order; K <= 4096 rows against the LDS copy of the keys).
__global__ __launch_bounds__(THREADS) void scales_kernel(const double* __restrict__ d, int K, float tau,
                                                         float* __restrict__ s, float* __restrict__ tau_out) {
  __shared__ uint32_t key[MAXROWS];
  __shared__ float tmed;
  float t = tau;
  if (tau == 0.f) {
    for (int i = threadIdx.x; i < K; i += THREADS) key[i] = sort_key((float)d[i]);
    __syncthreads();
    const int m = (K - 1) / 2;
    for (int i = threadIdx.x; i < K; i += THREADS)
      if (rank_below(key, K, i) == m) tmed = (float)d[i];  // the ranks are a permutation: one writer
    __syncthreads();
    t = tmed;
  }
  if (threadIdx.x == 0 && tau_out) *tau_out = t;
  for (int i = threadIdx.x; i < K; i += THREADS) {
    const float d32 = (float)d[i];
    s[i] = d32 != d32 ? 0.f : (d32 > t ? div_rn(t, d32) : 1.f);
  }
}

// W adjacent coordinates from p on, the rows streamed (stream_rows).
template <int W>
__device__ __forceinline__ void step_columns(const float* __restrict__ X, int K, int64_t ldx, int64_t p,
                                             const float* __restrict__ v, const float* ss,
                                             float* __restrict__ out) {
  float c[W], acc[W];
  load<W>(v + p, c);
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.f;
  stream_rows<W>(X + p, ldx, K, [](int k) { return k; }, [&](int k, const float(&x)[W]) {
    const float sk = uniform(ss[k]);
    if (sk != 0.f) {
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] = add_rn(acc[e], mul_rn(sub_rn(x[e], c[e]), sk));
    }
  });
  const float fk = (float)K;
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = add_rn(c[e], div_rn(acc[e], fk));
  store<W>(out + p, acc);
}

// One lane of the lane map (lane_columns) per workgroup lane.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void step_kernel(const float* __restrict__ X, int K, int64_t P, int64_t ldx,
                                                       const float* __restrict__ v, const float* __restrict__ s,
                                                       float* __restrict__ out) {
  __shared__ float ss[MAXROWS];
  for (int t = threadIdx.x; t < K; t += THREADS) ss[t] = s[t];
  __syncthreads();
  lane_columns<VEC>((int64_t)blockIdx.x * THREADS + threadIdx.x, P, [&](auto w, int64_t p) {
    step_columns<decltype(w)::value>(X, K, ldx, p, v, ss, out);
  });
}

// The workspace: the row_norms partials, then K distances, K scales and the
// second iterate vector, each 256-B aligned.
struct Layout {
  size_t part, norms, scales, vtmp, total;
  Layout(int64_t K, int64_t P) {
    part = 0;
    norms = align_up(flr_row_norms_workspace(K), 256);
    scales = norms + align_up((size_t)K * sizeof(double), 256);
    vtmp = scales + align_up((size_t)K * sizeof(float), 256);
    total = vtmp + align_up((size_t)P * sizeof(float), 256);
  }
};

}  // namespace cclip
}  // namespace flr

using namespace flr;

extern "C" size_t flr_centered_clip_workspace(int64_t K, int64_t P) {
  return (K < 1 || P < 1) ? 0 : cclip::Layout(K, P).total;
}

extern "C" int flr_centered_clip(const float* X, int64_t K, int64_t P, int64_t ldx, const float* v0, float tau,
                                 int64_t iters, float* out, double* norms_out, float* scales_out, float* tau_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !v0 || !out || K < 1 || P < 1 || ldx < P || iters < 1 || !(tau >= 0.f) || out == v0) return FLR_ERR_ARG;
  if (!workspace || workspace_bytes < flr_centered_clip_workspace(K, P) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255) != 0)
    return FLR_ERR_WORKSPACE;
  if (K > cclip::MAXROWS) return FLR_ERR_UNSUPPORTED;
  const bool vec = rows::vec_ok(X, v0, out, ldx);
  const int64_t nblocks = (rows::column_lanes(vec, P) + cclip::THREADS - 1) / cclip::THREADS;
  if (nblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const cclip::Layout lay(K, P);
  char* ws = static_cast<char*>(workspace);
  float* vtmp = reinterpret_cast<float*>(ws + lay.vtmp);
  const dim3 grid((unsigned)nblocks), block(cclip::THREADS);
  const float* cur = v0;
  for (int64_t l = 0; l < iters; ++l) {
    double* d = norms_out ? norms_out + l * K : reinterpret_cast<double*>(ws + lay.norms);
    float* s = scales_out ? scales_out + l * K : reinterpret_cast<float*>(ws + lay.scales);
    int rc = flr_row_norms(X, K, P, ldx, cur, 0, d, ws + lay.part, lay.norms, stream);
    if (rc != FLR_OK) return rc;
    hipLaunchKernelGGL(cclip::scales_kernel, dim3(1), block, 0, st, d, (int)K, tau, s, tau_out ? tau_out + l : nullptr);
    rc = launch_status("centered_clip scales");
    if (rc != FLR_OK) return rc;
    float* dst = (iters - 1 - l) % 2 == 0 ? out : vtmp;  // the last iterate lands in out
    if (vec)
      hipLaunchKernelGGL(cclip::step_kernel<true>, grid, block, 0, st, X, (int)K, P, ldx, cur, s, dst);
    else
      hipLaunchKernelGGL(cclip::step_kernel<false>, grid, block, 0, st, X, (int)K, P, ldx, cur, s, dst);
    rc = launch_status("centered_clip step");
    if (rc != FLR_OK) return rc;
    cur = dst;
  }
  return FLR_OK;
}
