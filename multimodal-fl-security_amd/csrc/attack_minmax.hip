// The Min-Max and Min-Sum colluding attacks (Shejwalkar, Houmansadr,
// "Manipulating the Byzantine: Optimizing Model Poisoning Attacks and Defenses
// for Federated Learning", NDSS 2021) on gfx950.  Every attacker submits
//   m = mu + gamma * p
// mu the benign mean, p a perturbation direction (-sigma, -sign(mu - g) or
// -(mu - g), g the round's global model), gamma the largest strength that keeps
// m no further from the benign rows than they are from each other:
//   Min-Max  max_i ||m - x_i||^2 <= R2 = max_ij ||x_i - x_j||^2
//   Min-Sum  sum_i ||m - x_i||^2 <= S  = max_i sum_j ||x_i - x_j||^2
// The strength comes from the round's own client matrix, not from a guess per
// defense (ALIE's z, IPM's epsilon: attack_colluding.hip).
//
// The paper searches gamma by halving, one pass over the matrix per probe.  Here
// it is solved in closed form: with d_i = mu - x_i, a_i = sum d_i^2, b_i = sum
// p d_i, c = sum p^2,  ||m - x_i||^2 = a_i + 2 gamma b_i + gamma^2 c, a quadratic
// per row (Min-Max: the smallest positive root over the rows) or one for the sum
// (Min-Sum).  The arithmetic is fixed in flr.h.
//
// Engine, all enqueued by the one C call (no host round trip, as
// flr_centered_clip):
//   1. mu, sigma        the mean/deviation pass of attack_colluding.hip with no
//                       row written: flr_collude_rows' bits
//   2. D                flr_pairwise_l2 (the Gram engine) on the benign rows
//   3. a_i, b_i, c      stats_kernel: ONE streaming pass over the benign rows for
//                       both sums (flr_row_norms + flr_row_dots would read X
//                       twice and form b_i by cancellation).  One lane per float4
//                       of coordinates, a workgroup per (column block, group of 16
//                       rows): p is formed on the fly from mu and sigma / g, the
//                       16 row loads are in flight together, each row has its own
//                       fp64 accumulators in registers.  Per-workgroup partials
//                       go to the workspace; finish_kernel sums them in a fixed
//                       order — no float atomics, run-to-run identical bits.
//                       HBM-bound: nb * P * 4 bytes read once.
//   4. gamma            solve_kernel, one workgroup, fp64: R2 and S from D, the
//                       closed form, gamma_out / stats_out
//   5. the rows         write_kernel: rows [0, nmal) <- mu + (float)gamma * p, one
//                       lane per float4; a NaN gamma skips it by a uniform branch
#include "rows_pass.h"

namespace flr {
namespace minmax {

using namespace rows;          // THREADS, the lane map, load / store (rows_pass.h)
constexpr int ROWS = 16;       // rows per workgroup = row loads in flight per lane
constexpr int MAXCB = 128;     // column blocks (partials per row)
constexpr int MAXROWS = 1024;  // benign rows: flr_pairwise_l2's limit (the one-workgroup solve would carry 4096)

// p of one coordinate; aux is sigma (FLR_PERTURB_STD) or g (the other two).
__device__ __forceinline__ float perturb(int pert, float mu, float aux) {
  if (pert == FLR_PERTURB_STD) return -aux;
  const float t = sub_rn(mu, aux);
  if (pert == FLR_PERTURB_UNIT) return -t;
  return -(t > 0.f ? 1.f : (t < 0.f ? -1.f : (t == 0.f ? 0.f : t)));  // sign(0) = 0, sign(NaN) = NaN
}

// W adjacent coordinates from p on, the group's ROWS rows from Xb on: the loads
// issue back to back (a row past the group's last benign row re-reads that row;
// its sums are dropped).
template <int W>
__device__ __forceinline__ void accumulate(const float* __restrict__ Xb, int last, int64_t ldx, int64_t p,
                                           const float* __restrict__ mu, const float* __restrict__ aux, int pert,
                                           double (&a)[ROWS], double (&b)[ROWS], double& c, bool with_c) {
  float m[W], x[W], pv[W];
  load<W>(mu + p, m);
  load<W>(aux + p, x);
  float t[ROWS][W];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) load<W>(Xb + (int64_t)min(i, last) * ldx + p, t[i]);
#pragma unroll
  for (int e = 0; e < W; ++e) {
    pv[e] = perturb(pert, m[e], x[e]);
    if (with_c) c += (double)pv[e] * (double)pv[e];  // wave-uniform: the first row group stores c
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float d = sub_rn(m[e], t[i][e]);
      a[i] += (double)d * (double)d;       // exact products, fp64 sums
      b[i] += (double)pv[e] * (double)d;
    }
  }
}

// grid (ncb, ceil(nb / ROWS)).  The lanes are the lane map's (rows_pass.h), split
// here by column block: block cb owns lanes [L cb / ncb, L (cb+1) / ncb), its
// float4 lanes first, so the two loops below stand in for lane_columns.
// part: [nb][ncb] partials of a, then of b (at nbp * ncb), then [ncb] of c.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void stats_kernel(const float* __restrict__ Xb, int nb, int64_t P, int64_t ldx,
                                                        const float* __restrict__ mu,
                                                        const float* __restrict__ aux, int pert, int ncb,
                                                        double* __restrict__ part) {
  __shared__ double red[THREADS / 64][2 * ROWS + 1];
  const int cb = blockIdx.x, r0 = blockIdx.y * ROWS;
  const int last = min(ROWS, nb - r0) - 1;  // the group's last benign row
  Xb += (int64_t)r0 * ldx;
  const bool with_c = blockIdx.y == 0;
  double a[ROWS], b[ROWS], c = 0.0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) a[i] = b[i] = 0.0;
  const int64_t nv = VEC ? P / 4 : 0;
  const int64_t L = VEC ? nv + (P & 3) : P;
  const int64_t q0 = L * cb / ncb, q1 = L * (cb + 1) / ncb;
  if constexpr (VEC) {
    const int64_t qv = q1 < nv ? q1 : nv;
    for (int64_t q = q0 + threadIdx.x; q < qv; q += THREADS) accumulate<4>(Xb, last, ldx, 4 * q, mu, aux, pert, a, b, c, with_c);
    for (int64_t q = (q0 > nv ? q0 : nv) + threadIdx.x; q < q1; q += THREADS)
      accumulate<1>(Xb, last, ldx, 4 * nv + (q - nv), mu, aux, pert, a, b, c, with_c);
  } else {
    for (int64_t q = q0 + threadIdx.x; q < q1; q += THREADS) accumulate<1>(Xb, last, ldx, q, mu, aux, pert, a, b, c, with_c);
  }
  // the workgroup's sums: lanes by xor-shuffle, then the four waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      a[i] += __shfl_xor(a[i], o, 64);
      b[i] += __shfl_xor(b[i], o, 64);
    }
    c += __shfl_xor(c, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    double* r = red[threadIdx.x >> 6];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      r[i] = a[i];
      r[ROWS + i] = b[i];
    }
    r[2 * ROWS] = c;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t > 2 * ROWS) return;
  double s = red[0][t];
  for (int w = 1; w < THREADS / 64; ++w) s += red[w][t];
  const int64_t nbp = (int64_t)gridDim.y * ROWS;
  if (t == 2 * ROWS) {
    if (blockIdx.y == 0) part[2 * nbp * ncb + cb] = s;
  } else {
    const int row = r0 + (t & (ROWS - 1));
    if (row < nb) part[(t < ROWS ? 0 : nbp * ncb) + (int64_t)row * ncb + cb] = s;
  }
}

// The partials summed in column-block order: stats = a[nb], b[nb], c.
__global__ void finish_kernel(const double* __restrict__ part, int nb, int64_t nbp, int ncb,
                              double* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > 2 * nb) return;
  const double* src = i < nb ? part + (int64_t)i * ncb
                             : (i < 2 * nb ? part + nbp * ncb + (int64_t)(i - nb) * ncb : part + 2 * nbp * ncb);
  double s = src[0];
  for (int k = 1; k < ncb; ++k) s += src[k];
  stats[i] = s;
}

// One workgroup, fp64 (flr.h's operation order).  stats: a[nb], b[nb], c in;
// R2, S and the bound used out.
__global__ __launch_bounds__(THREADS) void solve_kernel(const double* __restrict__ D, int nb, int objective,
                                                        double* __restrict__ stats, double* __restrict__ gamma_out) {
  __shared__ double r2s[THREADS], ss[THREADS], gs[THREADS];
  __shared__ int bad[THREADS];
  const int t = threadIdx.x;
  const double* a = stats;
  const double* b = stats + nb;
  const double c = stats[2 * nb];
  double r2 = 0.0, s = 0.0;
  int nan = 0;
  for (int i = t; i < nb; i += THREADS) {
    double row = 0.0;
    for (int j = 0; j < nb; ++j) {
      const double v = D[(int64_t)i * nb + j];
      const double v2 = v * v;
      r2 = nanmax(r2, v2);
      row += v2;
    }
    s = nanmax(s, row);
    nan |= (a[i] != a[i]) || (b[i] != b[i]);
  }
  r2s[t] = r2;
  ss[t] = s;
  bad[t] = nan;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      r2s[t] = nanmax(r2s[t], r2s[t + o]);
      ss[t] = nanmax(ss[t], ss[t + o]);
      bad[t] |= bad[t + o];
    }
    __syncthreads();
  }
  const double R2 = r2s[0], S = ss[0];
  const bool isnan = bad[0] || c != c || R2 != R2 || S != S;
  const bool solve = !isnan && c != 0.0;
  // Min-Max: every row's root, the smallest kept; a NaN root (inf - inf in R2 - a_i)
  // once seen is kept, as numpy's min: the order is free either way
  double g = __builtin_huge_val();
  if (solve && objective == FLR_MINMAX_MAX) {
    for (int i = t; i < nb; i += THREADS) {
      const double bi = b[i];
      double h = R2 - a[i];
      h = h < 0.0 ? 0.0 : h;
      const double gi = (sqrt(bi * bi + c * h) - bi) / c;
      g = nanmin(g, gi);
    }
  }
  gs[t] = g;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) gs[t] = nanmin(gs[t], gs[t + o]);
    __syncthreads();
  }
  if (t != 0) return;
  double gamma = 0.0;  // c == 0
  if (isnan) {
    gamma = __builtin_nan("");
  } else if (solve && objective == FLR_MINMAX_MAX) {
    gamma = gs[0];
  } else if (solve) {
    double A = 0.0, Bs = 0.0;
    for (int i = 0; i < nb; ++i) {
      A += a[i];
      Bs += b[i];
    }
    double h = S - A;
    h = h < 0.0 ? 0.0 : h;
    const double nc = (double)nb * c;
    gamma = (sqrt(Bs * Bs + nc * h) - Bs) / nc;
  }
  *gamma_out = gamma;
  stats[2 * nb + 1] = R2;
  stats[2 * nb + 2] = S;
  stats[2 * nb + 3] = objective == FLR_MINMAX_MAX ? R2 : S;
}

template <int W>
__device__ __forceinline__ void write_columns(float* __restrict__ X, int64_t ldx, int64_t nmal, int64_t p,
                                              const float* __restrict__ mu, const float* __restrict__ aux,
                                              int pert, float gf) {
  float m[W], x[W];
  load<W>(mu + p, m);
  load<W>(aux + p, x);
#pragma unroll
  for (int e = 0; e < W; ++e) m[e] = add_rn(m[e], mul_rn(gf, perturb(pert, m[e], x[e])));
  for (int64_t r = 0; r < nmal; ++r) store<W>(X + r * ldx + p, m);
}

// Rows [0, nmal) <- mu + (float)gamma * p; lanes as stats_kernel's.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void write_kernel(float* __restrict__ X, int64_t P, int64_t ldx, int64_t nmal,
                                                        const float* __restrict__ mu,
                                                        const float* __restrict__ aux, int pert,
                                                        const double* __restrict__ gamma) {
  const double g = *gamma;
  if (g != g) return;  // wave-uniform: the attackers' rows stay as they were
  const float gf = (float)g;
  lane_columns<VEC>((int64_t)blockIdx.x * THREADS + threadIdx.x, P, [&](auto w, int64_t p) {
    write_columns<decltype(w)::value>(X, ldx, nmal, p, mu, aux, pert, gf);
  });
}

// Column blocks: at least four 1024-coordinate steps per workgroup.
inline int column_blocks(int64_t P) {
  const int64_t n = (P + 4 * 4 * THREADS - 1) / (4 * 4 * THREADS);
  return (int)(n < 1 ? 1 : (n > MAXCB ? MAXCB : n));
}

// The workspace, every part 256-B aligned: mu and sigma first (flr.h says so),
// then D, the statistics partials, the statistics and gamma (used when the
// caller passes no stats_out / gamma_out), and flr_pairwise_l2's workspace.
struct Layout {
  size_t mu, sigma, D, part, stats, gamma, pw, total;
  Layout(int64_t nb, int64_t P) {
    const size_t nbp = (size_t)((nb + ROWS - 1) / ROWS * ROWS);
    mu = 0;
    sigma = mu + align_up((size_t)P * sizeof(float), 256);
    D = sigma + align_up((size_t)P * sizeof(float), 256);
    part = D + align_up((size_t)nb * nb * sizeof(double), 256);
    stats = part + align_up((2 * nbp + 1) * MAXCB * sizeof(double), 256);
    gamma = stats + align_up((2 * (size_t)nb + 4) * sizeof(double), 256);
    pw = gamma + 256;
    total = pw + align_up(flr_pairwise_l2_workspace(nb, P), 256);
  }
};

}  // namespace minmax
}  // namespace flr

using namespace flr;

extern "C" size_t flr_minmax_workspace(int64_t K, int64_t P, int64_t nmal) {
  return (K < 2 || P < 1 || nmal < 1 || nmal >= K) ? 0 : minmax::Layout(K - nmal, P).total;
}

extern "C" int flr_minmax_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal, int objective, int perturb,
                               const float* global, double* gamma_out, double* stats_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!X || K < 2 || nmal < 1 || nmal >= K || P < 1 || ldx < P ||
      (objective != FLR_MINMAX_MAX && objective != FLR_MINMAX_SUM) ||
      (perturb != FLR_PERTURB_STD && perturb != FLR_PERTURB_SIGN && perturb != FLR_PERTURB_UNIT) ||
      (perturb != FLR_PERTURB_STD && !global))
    return FLR_ERR_ARG;
  if (!workspace || workspace_bytes < flr_minmax_workspace(K, P, nmal) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255) != 0)
    return FLR_ERR_WORKSPACE;
  const int64_t nb = K - nmal;
  if (nb > minmax::MAXROWS) return FLR_ERR_UNSUPPORTED;
  const minmax::Layout lay(nb, P);
  char* ws = static_cast<char*>(workspace);
  float* mu = reinterpret_cast<float*>(ws + lay.mu);
  float* sigma = reinterpret_cast<float*>(ws + lay.sigma);
  double* D = reinterpret_cast<double*>(ws + lay.D);
  double* part = reinterpret_cast<double*>(ws + lay.part);
  double* stats = stats_out ? stats_out : reinterpret_cast<double*>(ws + lay.stats);
  double* gamma = gamma_out ? gamma_out : reinterpret_cast<double*>(ws + lay.gamma);
  const float* aux = perturb == FLR_PERTURB_STD ? sigma : global;
  const bool vec = rows::vec_ok(X, aux, ldx);
  const int64_t wblocks = (rows::column_lanes(vec, P) + minmax::THREADS - 1) / minmax::THREADS;
  if (wblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const float* Xb = X + nmal * ldx;
  // 1. mu, sigma: no row written
  int rc = collude::launch(X, K, P, ldx, nmal, collude::STATS_ONLY, 0.f, mu, sigma, st);
  if (rc != FLR_OK) return rc;
  // 2. D of the benign rows (nb is within its row limit: MAXROWS)
  rc = flr_pairwise_l2(Xb, nb, P, ldx, D, ws + lay.pw, workspace_bytes - lay.pw, stream);
  if (rc != FLR_OK) return rc;
  // 3. a_i, b_i, c
  const int ncb = minmax::column_blocks(P);
  const int ngroups = (int)((nb + minmax::ROWS - 1) / minmax::ROWS);
  const dim3 sgrid((unsigned)ncb, (unsigned)ngroups), block(minmax::THREADS);
  if (vec)
    hipLaunchKernelGGL(minmax::stats_kernel<true>, sgrid, block, 0, st, Xb, (int)nb, P, ldx, mu, aux, perturb, ncb,
                       part);
  else
    hipLaunchKernelGGL(minmax::stats_kernel<false>, sgrid, block, 0, st, Xb, (int)nb, P, ldx, mu, aux, perturb, ncb,
                       part);
  if ((rc = launch_status("minmax stats")) != FLR_OK) return rc;
  hipLaunchKernelGGL(minmax::finish_kernel, dim3((unsigned)((2 * nb + 1 + 255) / 256)), dim3(256), 0, st, part,
                     (int)nb, (int64_t)ngroups * minmax::ROWS, ncb, stats);
  if ((rc = launch_status("minmax finish")) != FLR_OK) return rc;
  // 4. gamma
  hipLaunchKernelGGL(minmax::solve_kernel, dim3(1), block, 0, st, D, (int)nb, objective, stats, gamma);
  if ((rc = launch_status("minmax solve")) != FLR_OK) return rc;
  // 5. the attackers' rows
  const dim3 wgrid((unsigned)wblocks);
  if (vec)
    hipLaunchKernelGGL(minmax::write_kernel<true>, wgrid, block, 0, st, X, P, ldx, nmal, mu, aux, perturb, gamma);
  else
    hipLaunchKernelGGL(minmax::write_kernel<false>, wgrid, block, 0, st, X, P, ldx, nmal, mu, aux, perturb, gamma);
  return launch_status("minmax write");
}
