// Divide-and-conquer (DnC; Shejwalkar, Houmansadr, "Manipulating the Byzantine:
// Optimizing Model Poisoning Attacks and Defenses for Federated Learning", NDSS
// 2021, Algorithm 2) on gfx950: the spectral defense for the paper's own Min-Max
// and Min-Sum attacks (attack_minmax.hip).  niters times: subsample b columns,
// center them over the clients, score every client by its squared projection on
// the top right singular vector of the centered K x b matrix C, drop the nremove
// highest scores; the kept set is the intersection, the aggregate its mean.
//
// The arithmetic is fixed (flr.h).  The singular vector is never formed: with
// the K x K Gram matrix G = C C^T (fp64, the products exact) and w = G u for the
// top eigenvector u of G, row i's projection is w_i / sqrt(u.w).
//
// Engine: all niters iterations are enqueued by the one C call, no host round
// trip (as flr_centered_clip): per iteration
//   gather    one lane per sampled column (generated on the device: a stratified
//             splitmix64 hash) and group of 16 rows, into the compact K x b
//             matrix; a non-finite value marks its row bad
//   center    one lane per column over the compact matrix: the good rows' fp32
//             sequential mean, then c = x - mu (bad rows: zeros)
//   gram      16 x 16 output tiles, 64-column LDS tiles, one fp64 lane per entry;
//             the columns cut into chunks (a function of K and b) so that a
//             small K still fills the device, each chunk summed in ascending
//             order, then the chunks' sums added in chunk order (rows_pass.h's
//             ColumnChunks and gram_reduce)
//   spectral  one workgroup: the power iteration on G (read through its
//             transpose — G is symmetric bit for bit — so the lanes' loads
//             coalesce; the sum over k split into wave-uniform slices combined
//             in slice order; K <= 128: a lane's entries of G stay in
//             registers), the scores, the rank-count selection and the AND into
//             keep; the last iteration counts and applies the fallback.
// The aggregate, the mean of the kept rows, is flr_rows_mean_keep (agg_mean.hip).
#include "rows_pass.h"

namespace flr {
namespace dnc {

using namespace rows;  // THREADS, STREAM, the row stream, block_reduce, the rank count (rows_pass.h)
constexpr int MAXK = 1024, MAXB = 65536, MAXITERS = 16, MAXPOWER = 1024;
constexpr int SPEC_THREADS = 1024;  // the spectral workgroup: one lane per client
constexpr int SPEC_WAVES = SPEC_THREADS / 64;
constexpr int GT = 16, GJ = 64;  // Gram: output tile edge, columns per LDS tile
constexpr int CENTER_THREADS = 64;

__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// The splitmix64 finaliser.
__device__ __forceinline__ uint64_t mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// Lane j of workgroup row y: sampled column j of iteration `it` — generated, or
// the caller's clamped into [0, P) — and its values in rows [16y, 16y + 16) into
// column j of the compact matrix C [K][b]: K * b scattered loads, 16 in flight
// per lane, spread over b / 256 x K / 16 workgroups.
__global__ __launch_bounds__(THREADS) void gather_kernel(const float* __restrict__ X, int K, int64_t P, int64_t ldx,
                                                         int b, uint64_t seed, int it,
                                                         const int64_t* __restrict__ cols, float* __restrict__ C,
                                                         int32_t* __restrict__ bad, int64_t* __restrict__ cols_out) {
  const int j = blockIdx.x * THREADS + threadIdx.x;
  if (j >= b) return;
  int64_t c;
  if (cols) {
    c = cols[j];
    c = c < 0 ? 0 : (c > P - 1 ? P - 1 : c);
  } else {
    const uint64_t lo = (uint64_t)j * (uint64_t)P / (uint64_t)b;
    const uint64_t hi = (uint64_t)(j + 1) * (uint64_t)P / (uint64_t)b;
    const uint64_t h = mix(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)it * (uint64_t)b + (uint64_t)j + 1));
    c = (int64_t)(lo + h % (hi - lo));
  }
  if (cols_out && blockIdx.y == 0) cols_out[j] = c;
  // one clamped group and no row loop: stream_rows would compile its full-group
  // and its partial-group body for a lane that runs one of them once
  const float* col = X + c;
  const int k0 = blockIdx.y * STREAM;
  float t[STREAM];
#pragma unroll
  for (int i = 0; i < STREAM; ++i) t[i] = col[(int64_t)min(k0 + i, K - 1) * ldx];
#pragma unroll
  for (int i = 0; i < STREAM; ++i) {
    if (k0 + i < K) {
      C[(int64_t)(k0 + i) * b + j] = t[i];
      if (non_finite(t[i])) atomicOr(&bad[k0 + i], 1);
    }
  }
}

// Lane j: column j of C <- x - mu over the good rows, zeros in the bad rows.  The
// adds are a chain, the loads are not: the rows are streamed (stream_rows), twice.
// One wave per workgroup, so that b columns reach b / 64 compute units.
__global__ __launch_bounds__(CENTER_THREADS) void center_kernel(float* __restrict__ C, int K, int b,
                                                         const int32_t* __restrict__ bad) {
  __shared__ int32_t sb[MAXK];
  __shared__ int ngood_s;
  if (threadIdx.x == 0) ngood_s = 0;
  __syncthreads();
  int good = 0;
  for (int i = threadIdx.x; i < K; i += CENTER_THREADS) {
    sb[i] = bad[i];
    good += sb[i] ? 0 : 1;
  }
  if (good) atomicAdd(&ngood_s, good);
  __syncthreads();
  const int j = blockIdx.x * CENTER_THREADS + threadIdx.x;
  if (j >= b) return;
  float* col = C + j;
  const auto row = [](int k) { return k; };
  float s = 0.f;
  stream_rows<1>(col, b, K, row, [&](int k, const float(&x)[1]) {
    if (!sb[k]) s = add_rn(s, x[0]);
  });
  const float mu = div_rn(s, (float)ngood_s);
  stream_rows<1>(col, b, K, row, [&](int k, const float(&x)[1]) {  // a group's loads precede its stores
    col[(int64_t)k * b] = sb[k] ? 0.f : sub_rn(x[0], mu);
  });
}

// The Gram sum's column chunks (ColumnChunks) over the 16 x 16 output tiles.
inline ColumnChunks gram_chunks(int64_t K, int64_t b) {
  const int64_t side = (K + GT - 1) / GT;
  return ColumnChunks(side * side, b, GJ);
}

// G = C C^T.  Workgroup (bx, by, bz): the 16 x 16 tile at rows 16*by, columns
// 16*bx, over the columns of chunk bz; lane (ty, tx) sums its entry over them in
// ascending order (the zeros that pad a tile add nothing) into dst + bz * K * K
// (G itself when there is one chunk).  The next tile's loads are in flight while
// this one is summed.  G[i][k] and G[k][i] see the same products in the same
// order: G is symmetric bit for bit.
__global__ __launch_bounds__(GT * GT) void gram_kernel(const float* __restrict__ C, int K, int b, int chunk,
                                                       double* __restrict__ dst) {
  __shared__ float As[GJ][GT + 1], Bs[GJ][GT + 1];
  constexpr int NR = GT * GJ / (GT * GT);  // rows of a tile per lane
  const int tx = threadIdx.x % GT, ty = threadIdx.x / GT;
  const int i0 = blockIdx.y * GT, k0 = blockIdx.x * GT;
  const int jj = threadIdx.x % GJ, r0 = threadIdx.x / GJ;
  const int jb = blockIdx.z * chunk, je = min(b, jb + chunk);
  float ra[NR], rb[NR];
  auto fetch = [&](int j0) {
    const int j = j0 + jj;
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      const int r = r0 + n * (GT * GT / GJ);
      ra[n] = (i0 + r < K && j < je) ? C[(int64_t)(i0 + r) * b + j] : 0.f;
      rb[n] = (k0 + r < K && j < je) ? C[(int64_t)(k0 + r) * b + j] : 0.f;
    }
  };
  double acc = 0.0;
  fetch(jb);
  for (int j0 = jb; j0 < je; j0 += GJ) {
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      As[jj][r0 + n * (GT * GT / GJ)] = ra[n];
      Bs[jj][r0 + n * (GT * GT / GJ)] = rb[n];
    }
    __syncthreads();
    if (j0 + GJ < je) fetch(j0 + GJ);
#pragma unroll 16
    for (int q = 0; q < GJ; ++q) acc = __builtin_fma((double)As[q][ty], (double)Bs[q][tx], acc);
    __syncthreads();
  }
  if (i0 + ty < K && k0 + tx < K) dst[(int64_t)blockIdx.z * K * K + (int64_t)(i0 + ty) * K + k0 + tx] = acc;
}

// Workgroup-wide reductions (block_reduce): every lane gets the same bits.
__device__ __forceinline__ double block_sum(double v, double* red) {
  return block_reduce<SPEC_WAVES>(v, red, [](double a, double o) { return a + o; });
}
__device__ __forceinline__ int block_count(int v, int* red) {
  return block_reduce<SPEC_WAVES>(v, red, [](int a, int o) { return a + o; });
}

// The power iteration from u (LDS, all MAXK entries defined and synchronised):
// power_iters times w = G u, u = w / ||w||, then w = G u, lam = u.w and lane t's
// score w_t^2 / lam.  False in the degenerate cases (a ||w|| of 0, lam <= 0), a
// result uniform over the workgroup.  Lane t works on row t % kb in slice t / kb
// of the k range (kb: K rounded up to whole waves, so a slice is wave-uniform);
// the slices' sums go through LDS (part) and are added in slice order; the
// workgroup sums' barriers also order the reuse of part.  REG (K <= 128: at
// least 8 slices, at most REG_PER entries of a row per lane): the lane's entries
// of G are loaded once and stay in registers over all the steps; otherwise they
// are read from memory (L2) at every step.  The same sums either way.
constexpr int REG_PER = 16;
template <bool REG>
__device__ __forceinline__ bool power_scores(const double* __restrict__ G, int K, int power_iters, double* u,
                                             double* part, double* red, double& score) {
  const int t = threadIdx.x;
  const int kb = (K + 63) / 64 * 64, ns = SPEC_THREADS / kb, per = (K + ns - 1) / ns;
  const int i = t % kb, s = t / kb, ke = min(K, (s + 1) * per);
  const bool mine = s < ns && i < K;
  double g[REG_PER];
  if constexpr (REG) {
#pragma unroll
    for (int q = 0; q < REG_PER; ++q) g[q] = (mine && s * per + q < ke) ? G[(int64_t)(s * per + q) * K + i] : 0.0;
  }
  double w = 0.0;
  for (int p = 0; p <= power_iters; ++p) {
    if (mine) {
      double a = 0.0;
      if constexpr (REG) {
#pragma unroll
        for (int q = 0; q < REG_PER; ++q)
          if (s * per + q < ke) a = __builtin_fma(g[q], u[s * per + q], a);
      } else {
#pragma unroll 8
        for (int k = s * per; k < ke; ++k) a = __builtin_fma(G[(int64_t)k * K + i], u[k], a);
      }
      part[s * kb + i] = a;
    }
    __syncthreads();
    w = 0.0;
    if (t < K)
      for (int q = 0; q < ns; ++q) w += part[q * kb + t];
    if (p == power_iters) break;  // the last product is the scores'
    const double nrm = sqrt(block_sum(w * w, red));
    if (nrm == 0.0) return false;
    if (t < K) u[t] = w / nrm;
    __syncthreads();
  }
  const double lam = block_sum(t < K ? u[t] * w : 0.0, red);
  if (lam <= 0.0) return false;
  score = w * w / lam;
  return true;
}

// Ascending order of the doubles as unsigned keys; NaN above +inf, a bad row
// above everything: NaN's shared key, all ones, moves one down to make room.
__device__ __forceinline__ uint64_t sort_key(double x, bool bad) {
  const uint64_t nan = 0xffffffffffffffffull, k = rows::sort_key(x);
  return bad ? nan : (k == nan ? nan - 1 : k);
}

// One workgroup, lane t = client t.  The scores of iteration `it` from G, its
// kept set ANDed into keep; `last`: the count, and the fallback to iteration 0's
// set (keep0) when the intersection is empty.
template <bool REG>
__global__ __launch_bounds__(SPEC_THREADS) void spectral_kernel(const double* __restrict__ G, int K,
                                                                const int32_t* __restrict__ bad, int nremove,
                                                                int power_iters, int it, int last,
                                                                int32_t* __restrict__ keep, int32_t* __restrict__ keep0,
                                                                int32_t* __restrict__ count,
                                                                double* __restrict__ scores_out,
                                                                int32_t* __restrict__ flags_out) {
  __shared__ double u[MAXK], part[SPEC_THREADS], red[SPEC_WAVES];
  __shared__ uint64_t key[MAXK];
  __shared__ int ired[SPEC_WAVES];
  const int t = threadIdx.x;
  const bool row = t < K;
  const bool isbad = row && bad[t] != 0;

  const double diag = row ? G[(int64_t)t * K + t] : -1.0;
  const double gaa = block_reduce<SPEC_WAVES>(diag, red, [](double a, double o) { return fmax(a, o); });
  // the lowest index of the largest entry
  const int a = block_reduce<SPEC_WAVES>(row && diag == gaa ? t : K, ired, [](int a, int o) { return min(a, o); });
  bool degenerate = a >= K || gaa == 0.0;
  double score = 0.0;
  if (!degenerate) {  // every branch below is uniform over the workgroup
    const double ga = row ? G[(int64_t)a * K + t] : 0.0;
    const double n0 = sqrt(block_sum(ga * ga, red));
    u[t] = row ? ga / n0 : 0.0;
    __syncthreads();
    degenerate = !power_scores<REG>(G, K, power_iters, u, part, red, score);
  }
  if (degenerate) score = 0.0;
  if (isbad) score = __builtin_huge_val();
  if (row) {
    key[t] = sort_key(score, isbad);
    if (scores_out) scores_out[t] = score;
  }
  __syncthreads();
  int kept = 0;
  if (row) kept = (!isbad && rank_below(key, K, t) < K - nremove) ? 1 : 0;
  const int first = row ? (it == 0 ? kept : keep0[t]) : 0;  // iteration 0's set
  int kp = row ? (it == 0 ? kept : (kept & (keep[t] != 0 ? 1 : 0))) : 0;
  if (row && it == 0 && !last) keep0[t] = kept;
  if (last) {
    int n = block_count(kp, ired);
    int flag = 0;
    if (n == 0) {
      flag = 1;
      kp = first;
      n = block_count(kp, ired);
    }
    if (t == 0) {
      *count = n;
      if (flags_out) *flags_out = flag;
    }
  }
  if (row) keep[t] = kp;
}

// The workspace: the compact K x b matrix, G, the column chunks' partial
// matrices (none for one chunk), the bad flags of every iteration (cleared by
// one memset per call) and iteration 0's kept set, each 256-B aligned.
struct Layout {
  size_t c, g, part, bad, keep0, total;
  Layout(int64_t K, int64_t b) {
    const ColumnChunks plan = gram_chunks(K, b);
    const size_t kk = (size_t)K * (size_t)K * sizeof(double);
    c = 0;
    g = align_up((size_t)K * (size_t)b * sizeof(float), 256);
    part = g + align_up(kk, 256);
    bad = part + (plan.splits > 1 ? align_up(kk * plan.splits, 256) : 0);
    keep0 = bad + align_up((size_t)MAXITERS * K * sizeof(int32_t), 256);
    total = keep0 + align_up((size_t)K * sizeof(int32_t), 256);
  }
};

}  // namespace dnc
}  // namespace flr

using namespace flr;

extern "C" size_t flr_dnc_workspace(int64_t K, int64_t b) {
  return (K < 1 || b < 1 || K > dnc::MAXK || b > dnc::MAXB) ? 0 : dnc::Layout(K, b).total;
}

extern "C" int flr_dnc_select(const float* X, int64_t K, int64_t P, int64_t ldx, int64_t b, int64_t niters,
                              int64_t nremove, int64_t power_iters, uint64_t seed, const int64_t* cols,
                              int32_t* keep, int32_t* count, double* scores_out, int64_t* cols_out,
                              int32_t* flags_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !keep || !count || K < 1 || b < 1 || b > P || ldx < P || niters < 1 || power_iters < 1 || nremove < 0 ||
      nremove > K - 1)
    return FLR_ERR_ARG;
  if (K > dnc::MAXK || b > dnc::MAXB || niters > dnc::MAXITERS || power_iters > dnc::MAXPOWER)
    return FLR_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < flr_dnc_workspace(K, b) || (reinterpret_cast<uintptr_t>(workspace) & 255) != 0)
    return FLR_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const dnc::Layout lay(K, b);
  char* ws = static_cast<char*>(workspace);
  float* C = reinterpret_cast<float*>(ws + lay.c);
  double* G = reinterpret_cast<double*>(ws + lay.g);
  double* part = reinterpret_cast<double*>(ws + lay.part);
  int32_t* bad_all = reinterpret_cast<int32_t*>(ws + lay.bad);
  int32_t* keep0 = reinterpret_cast<int32_t*>(ws + lay.keep0);
  const rows::ColumnChunks plan = dnc::gram_chunks(K, b);
  const dim3 block(dnc::THREADS);
  const dim3 gathergrid((unsigned)((b + dnc::THREADS - 1) / dnc::THREADS),
                        (unsigned)((K + dnc::STREAM - 1) / dnc::STREAM));
  const dim3 centergrid((unsigned)((b + dnc::CENTER_THREADS - 1) / dnc::CENTER_THREADS));
  const unsigned gt = (unsigned)((K + dnc::GT - 1) / dnc::GT);
  const bool reg = K <= 128;  // at least 8 k slices: at most REG_PER entries of a row of G per lane
  hipError_t e = hipMemsetAsync(bad_all, 0, (size_t)niters * K * sizeof(int32_t), st);
  if (e != hipSuccess) {
    set_last_error("dnc bad-row flags", e);
    return FLR_ERR_HIP;
  }
  for (int64_t it = 0; it < niters; ++it) {
    int32_t* bad = bad_all + it * K;
    hipLaunchKernelGGL(dnc::gather_kernel, gathergrid, block, 0, st, X, (int)K, P, ldx, (int)b, seed, (int)it,
                       cols ? cols + it * b : nullptr, C, bad, cols_out ? cols_out + it * b : nullptr);
    int rc = launch_status("dnc gather");
    if (rc != FLR_OK) return rc;
    hipLaunchKernelGGL(dnc::center_kernel, centergrid, dim3(dnc::CENTER_THREADS), 0, st, C, (int)K, (int)b, bad);
    rc = launch_status("dnc center");
    if (rc != FLR_OK) return rc;
    hipLaunchKernelGGL(dnc::gram_kernel, dim3(gt, gt, (unsigned)plan.splits), dim3(dnc::GT * dnc::GT), 0, st, C,
                       (int)K, (int)b, (int)plan.chunk, plan.splits > 1 ? part : G);
    rc = launch_status("dnc gram");
    if (rc != FLR_OK) return rc;
    if (plan.splits > 1) {
      // the partial matrices are symmetric bit for bit (gram_kernel): the one sum per pair is both entries
      rc = rows::gram_reduce(part, plan.splits, (int)K, G, st);
      if (rc != FLR_OK) return rc;
    }
    if (reg)
      hipLaunchKernelGGL(dnc::spectral_kernel<true>, dim3(1), dim3(dnc::SPEC_THREADS), 0, st, G, (int)K, bad,
                         (int)nremove, (int)power_iters, (int)it, it == niters - 1 ? 1 : 0, keep, keep0, count,
                         scores_out ? scores_out + it * K : nullptr, flags_out);
    else
      hipLaunchKernelGGL(dnc::spectral_kernel<false>, dim3(1), dim3(dnc::SPEC_THREADS), 0, st, G, (int)K, bad,
                         (int)nremove, (int)power_iters, (int)it, it == niters - 1 ? 1 : 0, keep, keep0, count,
                         scores_out ? scores_out + it * K : nullptr, flags_out);
    rc = launch_status("dnc spectral");
    if (rc != FLR_OK) return rc;
  }
  return FLR_OK;
}
