// The robust learning rate, RLR (Ozdayi, Kantarcioglu, Gel, "Defending against
// Backdoors in Federated Learning with Robust Learning Rate", AAAI 2021) on
// gfx950: per coordinate the clients vote with the sign of their update
//   votes[p] = #{k : x_k[p] > g[p]} - #{k : x_k[p] < g[p]}
// and where fewer than theta net votes agree the server's learning rate for that
// coordinate is negated: the aggregate moves away from an unopposed minority,
//   out[p] = g[p] + eta * (agg[p] - g[p])   |votes[p]| >= theta
//            g[p] - eta * (agg[p] - g[p])   otherwise
// agg any base aggregate.  The defense for the backdoor: its rows lie inside the
// benign spread (nothing for the row-level rules to reject), the harm sits on the
// coordinates where the honest clients have no common opinion.
//
// The arithmetic is fixed (flr.h): the vote is comparisons only, an exact
// integer; the step is three separately rounded fp32 ops (no FMA), and eta == 1
// on a passing coordinate hands the base aggregate's own bits through.
//
// Engine: three entries, each one enqueued kernel (and the 8-byte memset of the
// flip counter), no host round trip.  flr_sign_vote reads X once; flr_rlr_apply
// is a P-vector pass; flr_rlr_fedavg is both around flr_fedavg's accumulator in
// one pass over X — the vote costs compares on values the sum loads anyway, so
// the defense adds no second pass over the client matrix.  All are HBM-bound:
// one lane per float4 of coordinates with a scalar lane per coordinate of the
// P mod 4 tail, one lane per coordinate when a pointer is not 16-B aligned or
// ldx % 4 != 0 (rows_pass.h's lane map), the rows streamed with 16 loads in
// flight per lane (its stream_rows), the lanes striding over the lane map
// (grid_for).  The flip count is one block_reduce and one atomicAdd per workgroup.
#include "rows_pass.h"

#include <cmath>

namespace flr {
namespace rlr {

using namespace rows;          // THREADS, the lane map, the row stream, block_reduce (rows_pass.h)
constexpr int MAXROWS = 4096;  // the FedAvg weights in LDS; flr_fedavg's limit
constexpr int WAVES = THREADS / 64;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// W adjacent int32 from / to p, as rows::load / store.
template <int W>
__device__ __forceinline__ void load_i(const int32_t* __restrict__ p, int (&x)[W]) {
  if constexpr (W == 4) {
    const i32x4 t = *reinterpret_cast<const i32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = t[e];
  } else {
    x[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void store_i(int32_t* __restrict__ p, const int (&x)[W]) {
  if constexpr (W == 4) {
    i32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = x[e];
    *reinterpret_cast<i32x4*>(p) = t;
  } else {
    *p = x[0];
  }
}

// One client's vote on one coordinate: comparisons only.  A NaN on either side
// and -0 against +0 compare false both ways: 0.
__device__ __forceinline__ int vote(float x, float g) { return (x > g ? 1 : 0) - (x < g ? 1 : 0); }

// The step on one coordinate; returns 1 when the learning rate was negated.
__device__ __forceinline__ int step(float agg, float g, int votes, int theta, float eta, float& out) {
  const float ed = mul_rn(eta, sub_rn(agg, g));
  const bool pass = (votes < 0 ? -votes : votes) >= theta;
  out = pass ? (eta == 1.f ? agg : add_rn(g, ed)) : sub_rn(g, ed);
  return pass ? 0 : 1;
}

// The workgroup's flips -> *flipped: one atomicAdd per workgroup.
__device__ __forceinline__ void add_flips(int nflip, unsigned long long* flipped) {
  __shared__ int red[WAVES];
  const int total = block_reduce<WAVES>(nflip, red, [](int a, int b) { return a + b; });
  if (flipped && threadIdx.x == 0 && total != 0) atomicAdd(flipped, (unsigned long long)total);
}

// W adjacent coordinates from p on: the K rows streamed, W counters.
template <int W>
__device__ __forceinline__ void vote_columns(const float* __restrict__ X, int K, int64_t ldx, int64_t p,
                                             const float* __restrict__ g, int32_t* __restrict__ votes) {
  float c[W];
  int cnt[W];
  load<W>(g + p, c);
#pragma unroll
  for (int e = 0; e < W; ++e) cnt[e] = 0;
  stream_rows<W>(X + p, ldx, K, [](int k) { return k; }, [&](int, const float(&x)[W]) {
#pragma unroll
    for (int e = 0; e < W; ++e) cnt[e] += vote(x[e], c[e]);
  });
  store_i<W>(votes + p, cnt);
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void sign_vote_kernel(const float* __restrict__ X, int K, int64_t P, int64_t ldx,
                                                            const float* __restrict__ g,
                                                            int32_t* __restrict__ votes) {
  const int64_t lanes = VEC ? P / 4 + (P & 3) : P, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < lanes; q += stride)
    lane_columns<VEC>(q, P, [&](auto w, int64_t p) { vote_columns<decltype(w)::value>(X, K, ldx, p, g, votes); });
}

// agg and out may be one vector: a lane reads its coordinates before it writes them.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void apply_kernel(const float* agg, const float* __restrict__ g,
                                                        const int32_t* __restrict__ votes, int64_t P, int theta,
                                                        float eta, float* out, unsigned long long* flipped) {
  int nflip = 0;
  const int64_t lanes = VEC ? P / 4 + (P & 3) : P, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < lanes; q += stride)
    lane_columns<VEC>(q, P, [&](auto w, int64_t p) {
      constexpr int W = decltype(w)::value;
      float a[W], c[W], o[W];
      int v[W];
      load<W>(agg + p, a);
      load<W>(g + p, c);
      load_i<W>(votes + p, v);
#pragma unroll
      for (int e = 0; e < W; ++e) nflip += step(a[e], c[e], v[e], theta, eta, o[e]);
      store<W>(out + p, o);
    });
  add_flips(nflip, flipped);
}

// W adjacent coordinates from p on: flr_fedavg's accumulator and the counters on
// the same streamed rows, then the step.  Returns the coordinates flipped.
template <int W>
__device__ __forceinline__ int fedavg_columns(const float* __restrict__ X, int K, int64_t ldx, int64_t p,
                                              const float* wts, float total, const float* __restrict__ g, int theta,
                                              float eta, float* __restrict__ out, int32_t* __restrict__ votes_out) {
  float c[W], acc[W];
  int cnt[W];
  load<W>(g + p, c);
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.f, cnt[e] = 0;
  stream_rows<W>(X + p, ldx, K, [](int k) { return k; }, [&](int k, const float(&x)[W]) {
    const float wk = uniform(wts[k]);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      acc[e] = add_rn(acc[e], mul_rn(wk, x[e]));
      cnt[e] += vote(x[e], c[e]);
    }
  });
  int nflip = 0;
#pragma unroll
  for (int e = 0; e < W; ++e) nflip += step(div_rn(acc[e], total), c[e], cnt[e], theta, eta, acc[e]);
  store<W>(out + p, acc);
  if (votes_out) store_i<W>(votes_out + p, cnt);
  return nflip;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void rlr_fedavg_kernel(const float* __restrict__ X, int K, int64_t P, int64_t ldx,
                                                             const int64_t* __restrict__ n,
                                                             const float* __restrict__ g, int theta, float eta,
                                                             float* __restrict__ out, int32_t* __restrict__ votes_out,
                                                             unsigned long long* flipped) {
  __shared__ float wts[MAXROWS];
  __shared__ float total_f;
  for (int i = threadIdx.x; i < K; i += THREADS) wts[i] = (float)n[i];  // as fedavg_kernel (agg_mean.hip)
  if (threadIdx.x == 0) {
    int64_t tot = 0;
    for (int i = 0; i < K; ++i) tot += n[i];
    total_f = (float)tot;
  }
  __syncthreads();
  const float total = total_f;
  int nflip = 0;
  const int64_t lanes = VEC ? P / 4 + (P & 3) : P, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < lanes; q += stride)
    lane_columns<VEC>(q, P, [&](auto w, int64_t p) {
      nflip += fedavg_columns<decltype(w)::value>(X, K, ldx, p, wts, total, g, theta, eta, out, votes_out);
    });
  add_flips(nflip, flipped);
}

inline bool eta_ok(float eta) { return std::isfinite(eta) && eta > 0.f; }

// flipped <- 0 on the stream, ahead of the workgroups' adds.
inline int zero_flips(int64_t* flipped, hipStream_t st) {
  if (!flipped) return FLR_OK;
  const hipError_t e = hipMemsetAsync(flipped, 0, sizeof(int64_t), st);
  if (e != hipSuccess) {
    set_last_error("rlr flipped memset", e);
    return FLR_ERR_HIP;
  }
  return FLR_OK;
}

}  // namespace rlr
}  // namespace flr

using namespace flr;

extern "C" int flr_sign_vote(const float* X, int64_t K, int64_t P, int64_t ldx, const float* g, int32_t* votes,
                             void* stream) {
  if (!X || !g || !votes || K < 1 || P < 0 || ldx < P) return FLR_ERR_ARG;
  if (K > rlr::MAXROWS) return FLR_ERR_UNSUPPORTED;
  if (P == 0) return FLR_OK;
  const bool vec = rows::vec_ok(X, g, votes, ldx);
  const dim3 grid(rows::grid_for(rows::column_lanes(vec, P))), block(rlr::THREADS);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(rlr::sign_vote_kernel<true>, grid, block, 0, st, X, (int)K, P, ldx, g, votes);
  else
    hipLaunchKernelGGL(rlr::sign_vote_kernel<false>, grid, block, 0, st, X, (int)K, P, ldx, g, votes);
  return launch_status("sign_vote");
}

extern "C" int flr_rlr_apply(const float* agg, const float* g, const int32_t* votes, int64_t P, int64_t theta,
                             float eta, float* out, int64_t* flipped, void* stream) {
  if (!agg || !g || !votes || !out || P < 0 || theta < 0 || !rlr::eta_ok(eta) || out == g) return FLR_ERR_ARG;
  hipStream_t st = as_stream(stream);
  int rc = rlr::zero_flips(flipped, st);
  if (rc != FLR_OK || P == 0) return rc;
  const bool vec = rows::vec_ok(agg, g, votes, out);
  const dim3 grid(rows::grid_for(rows::column_lanes(vec, P))), block(rlr::THREADS);
  const int th = (int)(theta > 0x7fffffffLL ? 0x7fffffffLL : theta);  // |votes| is an int32 count
  unsigned long long* fl = reinterpret_cast<unsigned long long*>(flipped);
  if (vec)
    hipLaunchKernelGGL(rlr::apply_kernel<true>, grid, block, 0, st, agg, g, votes, P, th, eta, out, fl);
  else
    hipLaunchKernelGGL(rlr::apply_kernel<false>, grid, block, 0, st, agg, g, votes, P, th, eta, out, fl);
  return launch_status("rlr_apply");
}

extern "C" int flr_rlr_fedavg(const float* X, int64_t K, int64_t P, int64_t ldx, const int64_t* num_examples,
                              const float* g, int64_t theta, float eta, float* out, int32_t* votes_out,
                              int64_t* flipped, void* stream) {
  if (!X || !num_examples || !g || !out || K < 1 || P < 0 || ldx < P || theta < 0 || theta > K ||
      !rlr::eta_ok(eta) || out == g)
    return FLR_ERR_ARG;
  if (K > rlr::MAXROWS) return FLR_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  int rc = rlr::zero_flips(flipped, st);
  if (rc != FLR_OK || P == 0) return rc;
  const bool vec = rows::vec_ok(X, g, out, votes_out, ldx);
  const dim3 grid(rows::grid_for(rows::column_lanes(vec, P))), block(rlr::THREADS);
  unsigned long long* fl = reinterpret_cast<unsigned long long*>(flipped);
  if (vec)
    hipLaunchKernelGGL(rlr::rlr_fedavg_kernel<true>, grid, block, 0, st, X, (int)K, P, ldx, num_examples, g,
                       (int)theta, eta, out, votes_out, fl);
  else
    hipLaunchKernelGGL(rlr::rlr_fedavg_kernel<false>, grid, block, 0, st, X, (int)K, P, ldx, num_examples, g,
                       (int)theta, eta, out, votes_out, fl);
  return launch_status("rlr_fedavg");
}
