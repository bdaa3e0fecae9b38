// Model replacement (Bagdasaryan, Veit, Hua, Estrin, Shmatikov, "How To Backdoor
// Federated Learning", AISTATS 2020) on gfx950: the boosted backdoor.  The
// attackers (rows 0..f-1 of the exchanged client matrix, trained on triggered
// data) submit g + gamma_i * (x_i - g), g the round's global model: boosted so
// that the update survives the average, and shrunk back under the bound the
// server enforces — a norm bound (Sun et al. 2019) or the benign rows' largest
// mutual distance (the Min-Max criterion of attack_minmax.hip on each attacker's
// own direction: what Krum-type rules see).
//
// The arithmetic is fixed (flr.h).  Two calls, each enqueued on the stream with no
// host synchronisation:
//   flr_replace_strength  one workgroup, a lane per client, fp64: the benign
//                         statistic (rank-count median, maximum, ordered mean, or
//                         the largest squared distance from the centered Gram
//                         matrix), then each attacker's closed-form strength
//   flr_scale_rows_from   rows [0, n) <- c + (x - c) * gamma_i in place, fp32, a
//                         row with gamma_i == 1 or NaN never touched.  HBM-bound:
//                         a workgroup per 256 lanes of one row, a lane one float4
//                         of coordinates (2 * rows * P * 4 + P * 4 bytes from HBM;
//                         the center is re-read per row through the caches)
#include "rows_pass.h"

namespace flr {
namespace replace {

using namespace rows;       // THREADS, the lane map, load / store, block_reduce, the rank count
constexpr int MAXK = 1024;  // the strength kernel: one lane per client
constexpr int S_THREADS = 1024;
constexpr int S_WAVES = S_THREADS / 64;

// One workgroup, lane t = client t: t < f an attacker, t >= f benign row t - f.
__global__ __launch_bounds__(S_THREADS) void strength_kernel(const double* __restrict__ norms,
                                                             const double* __restrict__ G, int K, int f, double boost,
                                                             int mode, int stat, double rho,
                                                             double* __restrict__ gamma64, float* __restrict__ gamma32,
                                                             int32_t* __restrict__ status,
                                                             int32_t* __restrict__ flags) {
  __shared__ double val[MAXK];    // norm mode: the benign e_j; distance mode: G's diagonal
  __shared__ double sorted[MAXK];
  __shared__ uint64_t keys[MAXK];
  __shared__ double red[S_WAVES];
  __shared__ int ired[S_WAVES];
  const int t = threadIdx.x;
  const int nb = K - f;
  const bool attacker = t < f, benign = t >= f && t < K;
  if (mode == FLR_REPLACE_NONE) {  // wave-uniform
    if (attacker) {
      gamma64[t] = boost;
      gamma32[t] = (float)boost;
      status[t] = 0;
    }
    if (t == 0) *flags = 0;
    return;
  }

  // ---- the benign statistic B and the attacker's own e_i / a ----
  double B, own = 0.0;  // own: e_i (norm mode), a = G_ii (distance mode)
  bool own_bad = false;
  if (mode == FLR_REPLACE_NORM) {
    const double e = t < K ? norms[t] : 0.0;
    own = e;
    own_bad = attacker && !finite64(e);
    if (benign) {
      val[t - f] = e;
      keys[t - f] = sort_key(e);
    }
    __syncthreads();
    const int anynan = block_reduce<S_WAVES>((benign && e != e) ? 1 : 0, ired, [](int v, int o) { return v | o; });
    if (stat == FLR_REPLACE_MEDIAN) {
      if (benign) sorted[rank_below(keys, nb, t - f)] = e;
      __syncthreads();
      B = (nb & 1) ? sorted[nb / 2] : (sorted[nb / 2 - 1] + sorted[nb / 2]) / 2.0;
    } else if (stat == FLR_REPLACE_MAX) {
      B = block_reduce<S_WAVES>(benign ? e : 0.0, red, [](double v, double o) { return o > v ? o : v; });
    } else {
      double s = val[0];
      for (int j = 1; j < nb; ++j) s += val[j];
      B = s / (double)nb;
    }
    if (anynan) B = __builtin_nan("");
  } else {
    const double d = t < K ? G[(int64_t)t * K + t] : 0.0;
    own = d;
    own_bad = attacker && (!finite64(d) || (norms && !finite64(norms[t])));
    val[t] = d;
    __syncthreads();
    // benign lane j: the pairs (j, k), k > j; G_kj for G_jk (the lanes' loads coalesce)
    double d2 = 0.0;
    if (benign) {
      for (int k = t + 1; k < K; ++k) d2 = nanmax(d2, (d + val[k]) - 2.0 * G[(int64_t)k * K + t]);
    }
    B = block_reduce<S_WAVES>(d2, red, [](double v, double o) { return nanmax(v, o); });
  }
  const bool stat_bad = !finite64(B);  // the same bits in every lane

  // ---- the attackers' strengths ----
  double g = 1.0;
  int st = 3;
  if (attacker && !stat_bad && !own_bad) {
    if (own == 0.0) {
      g = boost;
      st = 0;
    } else if (mode == FLR_REPLACE_NORM) {
      const double bound = rho * B;
      if (boost * own <= bound) {
        g = boost;
        st = 0;
      } else {
        g = bound / own;
        st = 1;
      }
    } else {
      const double b2 = (rho * rho) * B;
      const double a = own;
      double m = __builtin_huge_val();
      bool infeasible = false;
      for (int j = f; j < K; ++j) {
        const double b = G[(int64_t)j * K + t];
        const double c = val[j] - b2;
        double disc = b * b - a * c;
        if (disc < 0.0) {
          infeasible = true;
          disc = 0.0;
        }
        m = nanmin(m, (b + sqrt(disc)) / a);
      }
      if (m < 0.0) {
        infeasible = true;
        m = 0.0;
      }
      g = m < boost ? m : boost;  // a NaN m: boost here, caught below
      st = infeasible ? 2 : (g < boost ? 1 : 0);
      if (m != m) g = m;
    }
    if (g != g) {
      g = 1.0;
      st = 3;
      own_bad = true;
    }
  }
  const int anybad = block_reduce<S_WAVES>(own_bad ? 1 : 0, ired, [](int v, int o) { return v | o; });
  if (attacker) {
    gamma64[t] = g;
    gamma32[t] = (float)g;
    status[t] = st;
  }
  if (t == 0) *flags = stat_bad ? 1 : (anybad ? 2 : 0);
}

// Row blockIdx.y, one lane of the lane map per thread (lane_columns).  The test of
// gamma is wave-uniform: a row with gamma == 1 or NaN is left by its workgroups
// before any load.  Measured against the column form (a lane walks the rows with
// 4 to 32 loads in flight and reads the center once): this one is 7 % faster
// (profiles/replace/); the center's re-reads come from the caches.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void scale_kernel(float* __restrict__ X, int64_t P, int64_t ldx,
                                                        const float* __restrict__ center,
                                                        const float* __restrict__ gamma) {
  const float gi = uniform(gamma[blockIdx.y]);
  if (gi == 1.f || gi != gi) return;
  float* x = X + (int64_t)blockIdx.y * ldx;
  lane_columns<VEC>((int64_t)blockIdx.x * THREADS + threadIdx.x, P, [&](auto w, int64_t p) {
    constexpr int W = decltype(w)::value;
    float xv[W], cv[W];
    load<W>(x + p, xv);
    load<W>(center + p, cv);
#pragma unroll
    for (int e = 0; e < W; ++e) xv[e] = add_rn(cv[e], mul_rn(sub_rn(xv[e], cv[e]), gi));
    store<W>(x + p, xv);
  });
}

}  // namespace replace
}  // namespace flr

using namespace flr;

extern "C" int flr_replace_strength(const double* norms, const double* G, int64_t K, int64_t f, double boost, int mode,
                                    int stat, double rho, double* gamma64, float* gamma32, int32_t* status,
                                    int32_t* flags, void* stream) {
  const double inf = __builtin_huge_val();
  if (!gamma64 || !gamma32 || !status || !flags || f < 1 || f >= K || !(boost > 0.0) || !(boost < inf) ||
      !(rho > 0.0) || !(rho < inf) ||
      (mode != FLR_REPLACE_NONE && mode != FLR_REPLACE_NORM && mode != FLR_REPLACE_DISTANCE) ||
      (stat != FLR_REPLACE_MEDIAN && stat != FLR_REPLACE_MAX && stat != FLR_REPLACE_MEAN) ||
      (mode == FLR_REPLACE_NORM && !norms) || (mode == FLR_REPLACE_DISTANCE && (!G || K - f < 2)))
    return FLR_ERR_ARG;
  if (K > replace::MAXK) return FLR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(replace::strength_kernel, dim3(1), dim3(replace::S_THREADS), 0, as_stream(stream), norms, G,
                     (int)K, (int)f, boost, mode, stat, rho, gamma64, gamma32, status, flags);
  return launch_status("replace_strength");
}

extern "C" int flr_scale_rows_from(float* X, int64_t K, int64_t P, int64_t ldx, const float* center,
                                   const float* gamma32, int64_t n, void* stream) {
  if (!X || !center || !gamma32 || K < 1 || P < 1 || ldx < P || n < 0 || n > K) return FLR_ERR_ARG;
  if (n == 0) return FLR_OK;
  if (n > 65535) return FLR_ERR_UNSUPPORTED;
  const bool vec = rows::vec_ok(X, center, ldx);
  const int64_t nblocks = (rows::column_lanes(vec, P) + replace::THREADS - 1) / replace::THREADS;
  if (nblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)nblocks, (unsigned)n), block(replace::THREADS);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(replace::scale_kernel<true>, grid, block, 0, st, X, P, ldx, center, gamma32);
  else
    hipLaunchKernelGGL(replace::scale_kernel<false>, grid, block, 0, st, X, P, ldx, center, gamma32);
  return launch_status("scale_rows_from");
}
