// Fang, Cao, Jia, Gong, "Local Model Poisoning Attacks to Byzantine-Robust
// Federated Learning" (USENIX Security 2020) on gfx950: the two full-knowledge
// attacks written against one aggregation rule each.  The attackers are rows
// 0..f-1 of the exchanged client matrix, s = sign(mu - g) the direction the
// benign clients moved in (mu their mean, g the round's global model).
//
//   flr_fang_krum_rows   every attacker submits g - lambda * s, lambda the largest
//                        of lambda0 * 2^-t for which Krum picks an attacker.  The
//                        paper runs a Krum over the attacked matrix per probe;
//                        here the probe is closed (flr.h): the benign rows'
//                        mutual distances come once from the centered Gram matrix
//                        G, the attackers' distances are sqrt(G_ii + 2 lambda b_i
//                        + lambda^2 c), b_i = <s, x_i - g>, c = <s, s>.
//     1. mu              attack_colluding.hip's mean pass, no row written
//     2. G               flr_rows_gram (agg_foolsgold.hip) on the benign rows
//     3. b_i, c, s       stats_kernel: one streaming pass over the benign rows, a
//                        workgroup per (column block, group of 16 rows), the 16
//                        row loads in flight together, fp64 accumulators in
//                        registers; finish_kernel adds the workgroups' partials
//                        in a fixed order (no float atomics).  nb * P * 4 bytes.
//     4. lambda          flr_fang_krum_strength: sort_kernel (a workgroup per
//                        benign row: its distances to the others, ranked, stored
//                        rank-major so the solver's lanes read them coalesced),
//                        then solve_kernel, one workgroup, a lane per benign row
//     5. the rows        write_kernel: rows [0, f) <- g - (float)lambda * s
//   flr_fang_trim_rows   per coordinate the attackers sit beyond the benign
//                        extreme on the side opposite s, at points drawn with a
//                        counter-based generator (Philox4x32-10, written out
//                        in philox.h: no RNG library) keyed by the coordinate's global
//                        index, so a column range gives the whole call's bits.
//                        One pass: a lane owns a float4 of coordinates, walks the
//                        benign rows with 16 loads in flight and writes the f
//                        rows.  (nb + f) * P * 4 bytes.
#include "philox.h"
#include "rows_pass.h"

namespace flr {
namespace fang {

using namespace rows;          // THREADS, the lane map, load / store, block_reduce, the rank count
constexpr int ROWS = 16;       // rows per workgroup = row loads in flight per lane
constexpr int MAXCB = 128;     // column blocks (partials per row)
constexpr int MAXROWS = 1024;  // benign rows: flr_rows_gram's limit, and one lane per row in the solver
constexpr int S_THREADS = 1024;
constexpr int S_WAVES = S_THREADS / 64;

// sign(0) = 0, sign(NaN) = NaN (FLR_PERTURB_SIGN's convention)
__device__ __forceinline__ float sign_of(float t) { return t > 0.f ? 1.f : (t < 0.f ? -1.f : (t == 0.f ? 0.f : t)); }

__device__ __forceinline__ double max0(double x) { return x < 0.0 ? 0.0 : x; }  // a NaN stays

// ---- stage 3: b_i, c and s ----

// W adjacent coordinates from p on, the group's ROWS rows from Xb on (a row past
// the group's last benign row re-reads that row; its sum is dropped).  first: the
// first row group also sums c and stores s.
template <int W>
__device__ __forceinline__ void accumulate(const float* __restrict__ Xb, int last, int64_t ldx, int64_t p,
                                           const float* __restrict__ mu, const float* __restrict__ g,
                                           float* __restrict__ s_out, double (&b)[ROWS], double& c, bool first) {
  float m[W], gv[W], sv[W];
  load<W>(mu + p, m);
  load<W>(g + p, gv);
  float t[ROWS][W];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) load<W>(Xb + (int64_t)min(i, last) * ldx + p, t[i]);
#pragma unroll
  for (int e = 0; e < W; ++e) {
    sv[e] = sign_of(sub_rn(m[e], gv[e]));
    if (first) c += (double)sv[e] * (double)sv[e];  // wave-uniform
  }
  if (first) store<W>(s_out + p, sv);
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
#pragma unroll
    for (int e = 0; e < W; ++e) b[i] += (double)sv[e] * (double)sub_rn(t[i][e], gv[e]);  // exact products, fp64 sums
  }
}

// grid (ncb, ceil(nb / ROWS)).  The lanes are the lane map's (rows_pass.h), split
// by column block as attack_minmax.hip's statistics pass: block cb owns lanes
// [L cb / ncb, L (cb+1) / ncb), its float4 lanes first.
// part: [nbp][ncb] partials of b, then [ncb] of c.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void stats_kernel(const float* __restrict__ Xb, int nb, int64_t P, int64_t ldx,
                                                        const float* __restrict__ mu, const float* __restrict__ g,
                                                        float* __restrict__ s_out, int ncb,
                                                        double* __restrict__ part) {
  __shared__ double red[THREADS / 64][ROWS + 1];
  const int cb = blockIdx.x, r0 = blockIdx.y * ROWS;
  const int last = min(ROWS, nb - r0) - 1;  // the group's last benign row
  Xb += (int64_t)r0 * ldx;
  const bool first = blockIdx.y == 0;
  double b[ROWS], c = 0.0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) b[i] = 0.0;
  const int64_t nv = VEC ? P / 4 : 0;
  const int64_t L = VEC ? nv + (P & 3) : P;
  const int64_t q0 = L * cb / ncb, q1 = L * (cb + 1) / ncb;
  if constexpr (VEC) {
    const int64_t qv = q1 < nv ? q1 : nv;
    for (int64_t q = q0 + threadIdx.x; q < qv; q += THREADS)
      accumulate<4>(Xb, last, ldx, 4 * q, mu, g, s_out, b, c, first);
    for (int64_t q = (q0 > nv ? q0 : nv) + threadIdx.x; q < q1; q += THREADS)
      accumulate<1>(Xb, last, ldx, 4 * nv + (q - nv), mu, g, s_out, b, c, first);
  } else {
    for (int64_t q = q0 + threadIdx.x; q < q1; q += THREADS) accumulate<1>(Xb, last, ldx, q, mu, g, s_out, b, c, first);
  }
  // the workgroup's sums: lanes by xor-shuffle, then the four waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) b[i] += __shfl_xor(b[i], o, 64);
    c += __shfl_xor(c, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    double* r = red[threadIdx.x >> 6];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) r[i] = b[i];
    r[ROWS] = c;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t > ROWS) return;
  double s = red[0][t];
  for (int w = 1; w < THREADS / 64; ++w) s += red[w][t];
  const int64_t nbp = (int64_t)gridDim.y * ROWS;
  if (t == ROWS) {
    if (first) part[nbp * ncb + cb] = s;
  } else if (r0 + t < nb) {
    part[(int64_t)(r0 + t) * ncb + cb] = s;
  }
}

// The partials summed in column-block order: bc = b[nb], c.
__global__ void finish_kernel(const double* __restrict__ part, int nb, int64_t nbp, int ncb, double* __restrict__ bc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nb) return;
  const double* src = i < nb ? part + (int64_t)i * ncb : part + nbp * ncb;
  double s = src[0];
  for (int k = 1; k < ncb; ++k) s += src[k];
  bc[i] = s;
}

// ---- stage 4: the strength ----

// Workgroup i: benign row i's distances to the nb - 1 others, ranked ascending
// (NaN last); Rt[rank * nb + i], rank-major: the solver's lanes walk the ranks.
__global__ __launch_bounds__(S_THREADS) void sort_kernel(const double* __restrict__ G, int nb,
                                                         double* __restrict__ Rt) {
  __shared__ uint64_t keys[MAXROWS];
  const int i = blockIdx.x, j = threadIdx.x;
  const bool live = j < nb && j != i;
  const int jj = j < i ? j : j - 1;
  double d = 0.0;
  if (live) {
    const double ei = G[(int64_t)i * nb + i], ej = G[(int64_t)j * nb + j];
    d = sqrt(max0((ei + ej) - 2.0 * G[(int64_t)i * nb + j]));
    keys[jj] = sort_key(d);
  }
  __syncthreads();
  if (live) Rt[(int64_t)rank_below(keys, nb - 1, jj) * nb + i] = d;
}

// One workgroup, lane t = benign row t (flr.h's operation order).
__global__ __launch_bounds__(S_THREADS) void solve_kernel(const double* __restrict__ G, const double* __restrict__ b,
                                                          const double* __restrict__ c,
                                                          const double* __restrict__ Rt, int K, int f,
                                                          double threshold, double* __restrict__ lambda64,
                                                          float* __restrict__ lambda32, int32_t* __restrict__ info,
                                                          double* __restrict__ stats_out) {
  __shared__ uint64_t keys[MAXROWS];
  __shared__ double sorted[MAXROWS];
  __shared__ double red[S_WAVES];
  __shared__ int ired[S_WAVES];
  const int t = threadIdx.x;
  const int nb = K - f, m = K - f - 2, na = K - 2 * f - 1;
  const bool live = t < nb;
  const double inf = __builtin_huge_val(), nan = __builtin_nan("");
  const double e = live ? G[(int64_t)t * nb + t] : 0.0;
  const double bi = live ? b[t] : 0.0;
  const double cc = *c;
  double Ti = 0.0;
  if (live) {
    for (int k = 0; k < m; ++k) Ti += Rt[(int64_t)k * nb + t];
  }
  const double T = block_reduce<S_WAVES>(live ? Ti : inf, red, [](double v, double o) { return nanmin(v, o); });
  const double E = block_reduce<S_WAVES>(live ? sqrt(e) : 0.0, red, [](double v, double o) { return nanmax(v, o); });
  const int anynan = block_reduce<S_WAVES>((e != e || bi != bi) ? 1 : 0, ired, [](int v, int o) { return v | o; });
  // every lane holds the same bits from here on: the branches are uniform
  double lam = nan, lam0 = nan, satt = nan, smin = nan;
  int status = 3, tt = 0;
  if (anynan || cc != cc || T != T) {
    status = 3;
  } else if (cc == 0.0) {
    lam = 0.0;
    status = 2;
  } else {
    const double rc = sqrt(cc);
    lam0 = T / ((double)na * rc) + E / rc;
    if (finite64(lam0)) {
      lam = lam0;
      for (;;) {
        if (lam <= threshold) {
          status = 1;
          break;
        }
        const double d = sqrt(max0((e + (2.0 * lam) * bi) + (lam * lam) * cc));
        __syncthreads();  // the last probe's reads of sorted are done
        if (live) keys[t] = sort_key(d);
        __syncthreads();
        if (live) sorted[rank_below(keys, nb, t)] = d;
        __syncthreads();
        satt = 0.0;
        for (int k = 0; k < na; ++k) satt += sorted[k];
        // the m smallest of r_t and f copies of d, ascending: r while r <= d, then the copies, then r again
        double si = 0.0;
        if (live) {
          int k = 0, used = 0;
          for (int step = 0; step < m; ++step) {  // k <= step < m < nb - 1: in bounds
            const double r = Rt[(int64_t)k * nb + t];
            if (used < f && !(r <= d)) {
              si += d;
              ++used;
            } else {
              si += r;
              ++k;
            }
          }
        }
        smin = block_reduce<S_WAVES>(live ? si : inf, red, [](double v, double o) { return nanmin(v, o); });
        if (satt <= smin) {
          status = 0;
          break;
        }
        lam *= 0.5;
        ++tt;
      }
    }
  }
  if (t != 0) return;
  *lambda64 = lam;
  *lambda32 = (float)lam;
  info[0] = status;
  info[1] = tt;
  if (stats_out) {
    stats_out[0] = lam0;
    stats_out[1] = T;
    stats_out[2] = E;
    stats_out[3] = satt;
    stats_out[4] = smin;
  }
}

// ---- stage 5: the rows ----

// Rows [0, nmal) <- g - (float)lambda * s; a NaN lambda leaves them (wave-uniform).
template <bool VEC>
__global__ __launch_bounds__(THREADS) void write_kernel(float* __restrict__ X, int64_t P, int64_t ldx, int64_t nmal,
                                                        const float* __restrict__ g, const float* __restrict__ s,
                                                        const float* __restrict__ lambda32) {
  const float lam = uniform(*lambda32);
  if (lam != lam) return;
  lane_columns<VEC>((int64_t)blockIdx.x * THREADS + threadIdx.x, P, [&](auto w, int64_t p) {
    constexpr int W = decltype(w)::value;
    float gv[W], sv[W];
    load<W>(g + p, gv);
    load<W>(s + p, sv);
#pragma unroll
    for (int e = 0; e < W; ++e) gv[e] = sub_rn(gv[e], mul_rn(lam, sv[e]));
    for (int64_t r = 0; r < nmal; ++r) store<W>(X + r * ldx + p, gv);
  });
}

// Column blocks: at least four 1024-coordinate steps per workgroup.
inline int column_blocks(int64_t P) {
  const int64_t n = (P + 4 * 4 * THREADS - 1) / (4 * 4 * THREADS);
  return (int)(n < 1 ? 1 : (n > MAXCB ? MAXCB : n));
}

inline size_t sorted_bytes(int64_t nb) { return align_up((size_t)nb * (size_t)(nb - 1) * sizeof(double), 256); }

// The workspace, every part 256-B aligned: mu and s first (flr.h says so).
struct Layout {
  size_t mu, s, G, gram, sorted, part, stats, lam64, lam32, info, total;
  Layout(int64_t nb, int64_t P) {
    const size_t nbp = (size_t)((nb + ROWS - 1) / ROWS * ROWS);
    mu = 0;
    s = mu + align_up((size_t)P * sizeof(float), 256);
    G = s + align_up((size_t)P * sizeof(float), 256);
    gram = G + align_up((size_t)nb * nb * sizeof(double), 256);
    sorted = gram + align_up(flr_rows_gram_workspace(nb, P), 256);
    part = sorted + sorted_bytes(nb);
    stats = part + align_up((nbp + 1) * MAXCB * sizeof(double), 256);
    lam64 = stats + align_up(((size_t)nb + 6) * sizeof(double), 256);
    lam32 = lam64 + 256;
    info = lam32 + 256;
    total = info + 256;
  }
};

inline bool threshold_ok(double th) { return th > 0.0 && th < __builtin_huge_val(); }

// flr_fang_krum_strength past its argument checks.
int strength(const double* G, const double* b, const double* c, int64_t K, int64_t f, double threshold,
             double* lambda64, float* lambda32, int32_t* info, double* stats_out, double* Rt, hipStream_t st) {
  const int nb = (int)(K - f);
  hipLaunchKernelGGL(sort_kernel, dim3((unsigned)nb), dim3(S_THREADS), 0, st, G, nb, Rt);
  const int rc = launch_status("fang_krum sort");
  if (rc != FLR_OK) return rc;
  hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(S_THREADS), 0, st, G, b, c, Rt, (int)K, (int)f, threshold, lambda64,
                     lambda32, info, stats_out);
  return launch_status("fang_krum solve");
}

// ---- the trimmed-mean attack ----

// The draws: word 0 of Philox4x32-10 (philox.h).
template <bool VEC>
__global__ __launch_bounds__(THREADS) void trim_kernel(float* __restrict__ X, int64_t nb, int64_t P, int64_t ldx,
                                                       int64_t nmal, const float* __restrict__ g, float bscale,
                                                       uint32_t k0, uint32_t k1, uint32_t draw_stream, int64_t col0) {
  lane_columns<VEC>((int64_t)blockIdx.x * THREADS + threadIdx.x, P, [&](auto w, int64_t p) {
    constexpr int W = decltype(w)::value;
    float sum[W], mn[W], mx[W], gv[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      sum[e] = 0.f;
      mn[e] = __builtin_huge_valf();   // the first row's value replaces both (a NaN column: s is NaN anyway)
      mx[e] = -__builtin_huge_valf();
    }
    load<W>(g + p, gv);
    stream_rows<W>(X + nmal * ldx + p, ldx, nb, [](int64_t k) { return k; }, [&](int64_t, const float(&x)[W]) {
#pragma unroll
      for (int e = 0; e < W; ++e) {
        sum[e] = add_rn(sum[e], x[e]);
        mn[e] = x[e] < mn[e] ? x[e] : mn[e];
        mx[e] = x[e] > mx[e] ? x[e] : mx[e];
      }
    });
    // every load of the column is done: the rows written are never among the rows read
    float near[W], span[W], fixed[W];
    bool draw[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float mu = div_rn(sum[e], (float)nb);
      const float t = sub_rn(mu, gv[e]);
      float far = 0.f;
      near[e] = 0.f;
      draw[e] = true;
      fixed[e] = 0.f;
      if (t > 0.f) {
        near[e] = mn[e];
        far = mn[e] > 0.f ? div_rn(mn[e], bscale) : mul_rn(mn[e], bscale);
      } else if (t < 0.f) {
        near[e] = mx[e];
        far = mx[e] > 0.f ? mul_rn(mx[e], bscale) : div_rn(mx[e], bscale);
      } else {
        draw[e] = false;
        fixed[e] = t == 0.f ? mu : t;
      }
      span[e] = sub_rn(far, near[e]);
    }
    for (int64_t i = 0; i < nmal; ++i) {
      float o[W];
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const uint64_t c = (uint64_t)(col0 + p + e);
        const uint32_t wd = philox_word0((uint32_t)c, (uint32_t)(c >> 32), (uint32_t)i, draw_stream, k0, k1);
        const float u = (float)(wd >> 8) * 0x1p-24f;  // 24 bits: exact
        o[e] = draw[e] ? add_rn(near[e], mul_rn(u, span[e])) : fixed[e];
      }
      store<W>(X + i * ldx + p, o);
    }
  });
}

}  // namespace fang
}  // namespace flr

using namespace flr;

extern "C" size_t flr_fang_krum_strength_workspace(int64_t K, int64_t nmal) {
  if (nmal < 1 || K < 2 * nmal + 3 || K - nmal > fang::MAXROWS) return 0;
  return fang::sorted_bytes(K - nmal);
}

extern "C" int flr_fang_krum_strength(const double* G, const double* b, const double* c, int64_t K, int64_t nmal,
                                      double threshold, double* lambda64, float* lambda32, int32_t* info,
                                      double* stats_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!G || !b || !c || !lambda64 || !lambda32 || !info || nmal < 1 || !fang::threshold_ok(threshold))
    return FLR_ERR_ARG;
  if (K < 2 * nmal + 3) return FLR_ERR_KRUM_N;
  if (K - nmal > fang::MAXROWS) return FLR_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < flr_fang_krum_strength_workspace(K, nmal) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255) != 0)
    return FLR_ERR_WORKSPACE;
  return fang::strength(G, b, c, K, nmal, threshold, lambda64, lambda32, info, stats_out,
                        static_cast<double*>(workspace), as_stream(stream));
}

extern "C" size_t flr_fang_krum_workspace(int64_t K, int64_t P, int64_t nmal) {
  if (P < 1 || nmal < 1 || K < 2 * nmal + 3 || K - nmal > fang::MAXROWS) return 0;
  return fang::Layout(K - nmal, P).total;
}

extern "C" int flr_fang_krum_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal, const float* global,
                                  double threshold, double* lambda_out, int32_t* info_out, double* stats_out,
                                  double* gram_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !global || K < 2 || nmal < 1 || nmal >= K || P < 1 || ldx < P || !fang::threshold_ok(threshold))
    return FLR_ERR_ARG;
  if (K < 2 * nmal + 3) return FLR_ERR_KRUM_N;
  const int64_t nb = K - nmal;
  if (nb > fang::MAXROWS) return FLR_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < flr_fang_krum_workspace(K, P, nmal) ||
      (reinterpret_cast<uintptr_t>(workspace) & 255) != 0)
    return FLR_ERR_WORKSPACE;
  const fang::Layout lay(nb, P);
  char* ws = static_cast<char*>(workspace);
  float* mu = reinterpret_cast<float*>(ws + lay.mu);
  float* s = reinterpret_cast<float*>(ws + lay.s);
  double* G = gram_out ? gram_out : reinterpret_cast<double*>(ws + lay.G);
  double* Rt = reinterpret_cast<double*>(ws + lay.sorted);
  double* part = reinterpret_cast<double*>(ws + lay.part);
  double* stats = stats_out ? stats_out : reinterpret_cast<double*>(ws + lay.stats);
  double* lam64 = lambda_out ? lambda_out : reinterpret_cast<double*>(ws + lay.lam64);
  float* lam32 = reinterpret_cast<float*>(ws + lay.lam32);
  int32_t* info = info_out ? info_out : reinterpret_cast<int32_t*>(ws + lay.info);
  const bool vec = rows::vec_ok(X, global, ldx);
  const int64_t wblocks = (rows::column_lanes(vec, P) + fang::THREADS - 1) / fang::THREADS;
  if (wblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const float* Xb = X + nmal * ldx;
  // 1. mu: no row written
  int rc = collude::launch(X, K, P, ldx, nmal, collude::STATS_ONLY, 0.f, mu, nullptr, st);
  if (rc != FLR_OK) return rc;
  // 2. G of the benign rows about g
  rc = flr_rows_gram(Xb, nb, P, ldx, global, G, ws + lay.gram, lay.sorted - lay.gram, stream);
  if (rc != FLR_OK) return rc;
  // 3. b_i, c, s
  const int ncb = fang::column_blocks(P);
  const int ngroups = (int)((nb + fang::ROWS - 1) / fang::ROWS);
  const dim3 sgrid((unsigned)ncb, (unsigned)ngroups), block(fang::THREADS);
  if (vec)
    hipLaunchKernelGGL(fang::stats_kernel<true>, sgrid, block, 0, st, Xb, (int)nb, P, ldx, mu, global, s, ncb, part);
  else
    hipLaunchKernelGGL(fang::stats_kernel<false>, sgrid, block, 0, st, Xb, (int)nb, P, ldx, mu, global, s, ncb, part);
  if ((rc = launch_status("fang_krum stats")) != FLR_OK) return rc;
  hipLaunchKernelGGL(fang::finish_kernel, dim3((unsigned)((nb + 1 + 255) / 256)), dim3(256), 0, st, part, (int)nb,
                     (int64_t)ngroups * fang::ROWS, ncb, stats);
  if ((rc = launch_status("fang_krum finish")) != FLR_OK) return rc;
  // 4. lambda
  rc = fang::strength(G, stats, stats + nb, K, nmal, threshold, lam64, lam32, info, stats + nb + 1, Rt, st);
  if (rc != FLR_OK) return rc;
  // 5. the attackers' rows
  const dim3 wgrid((unsigned)wblocks);
  if (vec)
    hipLaunchKernelGGL(fang::write_kernel<true>, wgrid, block, 0, st, X, P, ldx, nmal, global, s, lam32);
  else
    hipLaunchKernelGGL(fang::write_kernel<false>, wgrid, block, 0, st, X, P, ldx, nmal, global, s, lam32);
  return launch_status("fang_krum write");
}

extern "C" int flr_fang_trim_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal, const float* global,
                                  float b, uint64_t seed, uint32_t draw_stream, int64_t col0, void* stream) {
  if (!X || !global || K < 2 || nmal < 1 || nmal >= K || P < 1 || ldx < P || !(b > 1.f) ||
      !(b < __builtin_huge_valf()) || col0 < 0 || col0 > INT64_MAX - P)
    return FLR_ERR_ARG;
  const bool vec = rows::vec_ok(X, global, ldx);
  const int64_t nblocks = (rows::column_lanes(vec, P) + fang::THREADS - 1) / fang::THREADS;
  if (nblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)nblocks), block(fang::THREADS);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(fang::trim_kernel<true>, grid, block, 0, st, X, K - nmal, P, ldx, nmal, global, b, k0, k1,
                       draw_stream, col0);
  else
    hipLaunchKernelGGL(fang::trim_kernel<false>, grid, block, 0, st, X, K - nmal, P, ldx, nmal, global, b, k0, k1,
                       draw_stream, col0);
  return launch_status("fang_trim");
}
