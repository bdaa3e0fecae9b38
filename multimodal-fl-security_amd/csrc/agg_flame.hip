// FLAME (Nguyen et al., "FLAME: Taming Backdoors in Federated Learning", USENIX
// Security 2022, Algorithm 1) on gfx950: the backdoor defense.  The clients are
// clustered by the cosine distances of their updates, the majority cluster is
// admitted, its updates are clipped to the median update norm and averaged, and
// Gaussian noise scaled by that median is added.
//
// The arithmetic is fixed (flr.h).  Four calls, each enqueued on the stream with
// no host synchronisation:
//   flr_rows_gram          G = U U^T over all P coordinates, fp64, exact products
//                          (agg_foolsgold.hip)
//   flr_flame_select       one workgroup, a lane per client: distances,
//                          clustering, the median norm, the clipped weights, sigma
//   flr_rows_combine_from  out = center + sum_i beta_i * (x_i - center); rejected
//                          rows (beta_i == 0) are not read (agg_foolsgold.hip)
//   flr_add_gaussian       out += sigma * z in place, z from Philox4x32-10 and
//                          Box-Muller; 8 * P bytes
//
// The clustering.  The paper calls HDBSCAN(min_cluster_size = m = K/2 + 1,
// min_samples = 1, allow_single_cluster = True) on the cosine distances.  Two
// facts give that call a closed form:
//   - the core distance of a point is at most its distance to anyone, so the
//     mutual reachability distance is d_ij itself: the hierarchy is single linkage;
//   - with 2 m > K the condensed tree can never split into two clusters of m
//     points, so the one selected cluster is the first single-linkage component
//     that reaches m points.
// t* = the smallest t for which the graph with the edges {d_ij <= t} has a
// component of at least m good rows; that component (unique) is admitted.  Edges
// of equal weight enter together: no tie-breaking order can change the result.
// Given the same G bits a numpy restatement gives keep, t*, S, L, beta and sigma
// bit for bit (fp64 + - * / sqrt only, each rounded on its own).
//
// select_kernel.  Prim's minimum spanning tree over the implicit distance matrix:
// lane j keeps the key (its smallest distance to the tree) and the tree vertex
// that gave it; a step picks the smallest key of the lanes outside the tree (a
// wave butterfly, then the waves' results through LDS: one barrier per step, the
// LDS cells alternate between two sets), the picked lane records its edge, and
// every lane outside reads its entry of the picked row of G (coalesced) and
// lowers its key.  The keys are the distances as ordered unsigned integers
// (sort_key), NaN above everything: a NaN distance is no edge, and when no edge
// leaves the tree (bad rows aside that takes NaN distances) the lowest row
// outside starts a new tree with an edge that never merges.  The components of
// any minimum spanning tree cut at t are the components of the threshold graph,
// so ties in Prim's choice cannot change the answer.  The K - 1 tree edges are
// ranked in LDS; lane 0 merges them level by level (union by size, path halving)
// until a component holds m rows; every lane then finds its root.  The workgroup
// holds ceil(K / 64) waves.
#include "philox.h"
#include "rows_pass.h"

namespace flr {
namespace flame {

using namespace rows;  // THREADS, load / store, uniform, finite64, sort_key, rank_below
constexpr int MAXK = 1024;
constexpr int MAXWAVES = MAXK / 64;
constexpr uint64_t NO_EDGE = 0xffffffffffffffffull;  // sort_key of a NaN

// The double whose sort_key is k (k not NO_EDGE).
__device__ __forceinline__ double key_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ int find_root(const int* parent, int x) {
  while (parent[x] != x) x = parent[x];
  return x;
}

__global__ __launch_bounds__(MAXK) void select_kernel(const double* __restrict__ G, const double* __restrict__ norms,
                                                      int K, int m, double lambda, int32_t* __restrict__ keep,
                                                      float* __restrict__ beta, float* __restrict__ sigma,
                                                      double* __restrict__ stats, int32_t* __restrict__ flags) {
  __shared__ double nrm[MAXK];
  __shared__ uint64_t ew[MAXK];  // the tree edges' keys in Prim's order; then the median's keys
  __shared__ uint64_t sw[MAXK];  // the edges ranked by key
  __shared__ int eu[MAXK], ev[MAXK], su[MAXK], sv[MAXK];
  __shared__ int parent[MAXK], csize[MAXK];
  __shared__ uint64_t rkey[2][MAXWAVES];
  __shared__ int ridx[2][MAXWAVES];
  __shared__ int ired[MAXWAVES];
  __shared__ double median;
  __shared__ int found_root, found_size;
  __shared__ double found_t;

  const int t = threadIdx.x;
  const int nwaves = blockDim.x >> 6, wave = t >> 6;
  const bool row = t < K;
  const double gtt = row ? G[(int64_t)t * K + t] : 0.0;
  const bool bad = row && !finite64(gtt);
  const bool good = row && !bad;
  const double nt = row ? sqrt(gtt) : 0.0;
  nrm[t] = nt;
  parent[t] = t;
  csize[t] = 1;

  // the good rows' count, the bad rows' presence (every lane gets the same values)
  int cnt = good ? 1 : 0, anybad = bad ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    anybad |= __shfl_xor(anybad, o);
  }
  if ((t & 63) == 0) ired[wave] = cnt | (anybad << 16);
  __syncthreads();
  int ngood = 0;
  anybad = 0;
  for (int w = 0; w < nwaves; ++w) {
    ngood += ired[w] & 0xffff;
    anybad |= ired[w] >> 16;
  }

  // ---- Prim: step s picks vertex s of the order; from step 1 on it brings edge s - 1 ----
  uint64_t key = NO_EDGE;
  int par = t;
  bool outside = good;
  for (int s = 0; s < ngood; ++s) {
    uint64_t bk = NO_EDGE;
    int bi = outside ? t : 0x7fffffff;  // a lane outside the tree beats every other lane, NO_EDGE key or not
    if (outside) bk = key;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint64_t ok = (uint64_t)__shfl_xor((long long)bk, o);
      const int oi = __shfl_xor(bi, o);
      if (ok < bk || (ok == bk && oi < bi)) {
        bk = ok;
        bi = oi;
      }
    }
    const int b = s & 1;
    if ((t & 63) == 0) {
      rkey[b][wave] = bk;
      ridx[b][wave] = bi;
    }
    __syncthreads();
    bk = rkey[b][0];
    bi = ridx[b][0];
    for (int w = 1; w < nwaves; ++w) {
      const uint64_t ok = rkey[b][w];
      const int oi = ridx[b][w];
      if (ok < bk || (ok == bk && oi < bi)) {
        bk = ok;
        bi = oi;
      }
    }
    // bi < K: ngood - s good rows are still outside
    if (t == bi) {
      outside = false;
      if (s > 0) {
        ew[s - 1] = key;
        eu[s - 1] = t;
        ev[s - 1] = par;
      }
    }
    if (outside) {
      const double nv = nrm[bi];
      const double g = G[(int64_t)bi * K + t];
      const double d = (nt == 0.0 || nv == 0.0) ? 1.0 : 1.0 - g / (nt * nv);
      const uint64_t dk = sort_key(d);
      if (dk < key) {
        key = dk;
        par = bi;
      }
    }
  }
  __syncthreads();

  // ---- the edges by level ----
  const int nedges = ngood > 0 ? ngood - 1 : 0;
  if (t < nedges) {
    const int r = rank_below(ew, nedges, t);
    sw[r] = ew[t];
    su[r] = eu[t];
    sv[r] = ev[t];
  }
  __syncthreads();
  if (t == 0) {
    int root = -1, size = 0;
    double tstar = __builtin_huge_val();
    if (m == 1 && ngood >= 1) {  // K == 1
      root = 0;
      size = 1;
      tstar = 0.0;
    } else {
      int best = 0, broot = -1, e = 0;
      while (e < nedges && sw[e] != NO_EDGE) {
        const uint64_t w = sw[e];
        for (; e < nedges && sw[e] == w; ++e) {
          int a = su[e], c = sv[e];
          while (parent[a] != a) a = parent[a] = parent[parent[a]];
          while (parent[c] != c) c = parent[c] = parent[parent[c]];
          if (a == c) continue;  // never in a tree; kept for safety
          if (csize[a] < csize[c]) {
            const int x = a;
            a = c;
            c = x;
          }
          parent[c] = a;
          csize[a] += csize[c];
          if (csize[a] > best) {
            best = csize[a];
            broot = a;
          }
        }
        if (best >= m) {
          root = broot;
          size = best;
          tstar = key_value(w);
          break;
        }
      }
    }
    found_root = root;
    found_size = size;
    found_t = tstar;
  }
  __syncthreads();
  const int root = found_root, L = found_size;
  const bool admitted = good && root >= 0 && find_root(parent, t) == root;

  // ---- the clipping bound: the lower median of e over all K rows ----
  const double et = row ? (norms ? norms[t] : nt) : 0.0;
  if (row) ew[t] = sort_key(et);
  __syncthreads();
  if (row && rank_below(ew, K, t) == (K - 1) / 2) median = et;
  __syncthreads();
  const double S = median;
  if (row) {
    const double gamma = et > S ? S / et : 1.0;
    keep[t] = admitted ? 1 : 0;
    beta[t] = admitted ? (float)(gamma / (double)L) : 0.f;
  }
  if (t == 0) {
    *sigma = root >= 0 ? (float)(lambda * S) : 0.f;
    if (stats) {
      stats[0] = S;
      stats[1] = found_t;
      stats[2] = (double)L;
    }
    if (flags) *flags = (root >= 0 ? 0 : 1) | (anybad ? 2 : 0);
  }
}

// ---- flr_add_gaussian ----

// Box-Muller on two Philox words.
__device__ __forceinline__ void normal_pair(uint32_t wa, uint32_t wb, float& za, float& zb) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;  // 24 bits + 1: exact, in (0, 1]
  const float u2 = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(mul_rn(-2.f, logf(u1)));
  const float a = mul_rn(6.2831853071795864769f, u2);
  za = mul_rn(r, cosf(a));
  zb = mul_rn(r, sinf(a));
}

// Lane q: the Philox block c = c_first + q, the coordinates 4c - col0 + {0, 1, 2, 3}
// of v that lie in [0, P).  VEC: a whole block inside is one 16-byte access.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void gaussian_kernel(float* __restrict__ v, int64_t P,
                                                           const float* __restrict__ sigma, uint32_t k0, uint32_t k1,
                                                           uint32_t draw_stream, int64_t col0, int64_t c_first,
                                                           int64_t nblocks) {
  const float s = uniform(*sigma);
  if (s == 0.f) return;
  const int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (q >= nblocks) return;
  const uint64_t c = (uint64_t)(c_first + q);
  const int64_t k = (int64_t)(4 * c) - col0;  // >= -3
  uint32_t w0 = (uint32_t)c, w1 = (uint32_t)(c >> 32), w2 = 0u, w3 = draw_stream;
  philox4x32_10(w0, w1, w2, w3, k0, k1);
  float z[4];
  normal_pair(w0, w1, z[0], z[1]);
  normal_pair(w2, w3, z[2], z[3]);
  if (VEC && k >= 0 && k + 3 < P) {
    float x[4];
    load<4>(v + k, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = add_rn(x[j], mul_rn(s, z[j]));
    store<4>(v + k, x);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j >= 0 && k + j < P) v[k + j] = add_rn(v[k + j], mul_rn(s, z[j]));
  }
}

}  // namespace flame
}  // namespace flr

using namespace flr;

extern "C" int flr_flame_select(const double* G, const double* norms, int64_t K, int64_t m, double lambda,
                                int32_t* keep, float* beta, float* sigma, double* stats, int32_t* flags,
                                void* stream) {
  if (!G || !keep || !beta || !sigma || K < 1 || m > K || m < 1 || 2 * m <= K || !(lambda >= 0.0) ||
      !(lambda < __builtin_huge_val()))
    return FLR_ERR_ARG;
  if (K > flame::MAXK) return FLR_ERR_UNSUPPORTED;
  const unsigned threads = (unsigned)((K + 63) / 64 * 64);
  hipLaunchKernelGGL(flame::select_kernel, dim3(1), dim3(threads), 0, as_stream(stream), G, norms, (int)K, (int)m,
                     lambda, keep, beta, sigma, stats, flags);
  return launch_status("flame_select");
}

extern "C" int flr_add_gaussian(float* v, int64_t P, const float* sigma, uint64_t seed, uint32_t draw_stream,
                                int64_t col0, void* stream) {
  if (!v || !sigma || P < 0 || col0 < 0 || col0 > INT64_MAX - P) return FLR_ERR_ARG;
  if (P == 0) return FLR_OK;
  const int64_t c_first = col0 >> 2;
  const int64_t nblocks = ((col0 + P - 1) >> 2) - c_first + 1;
  const int64_t groups = (nblocks + flame::THREADS - 1) / flame::THREADS;
  if (groups > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(v);
  const bool vec = (addr & 3) == 0 && (((uint64_t)(addr >> 2) - (uint64_t)col0) & 3) == 0;
  const dim3 grid((unsigned)groups), block(flame::THREADS);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(flame::gaussian_kernel<true>, grid, block, 0, st, v, P, sigma, k0, k1, draw_stream, col0,
                       c_first, nblocks);
  else
    hipLaunchKernelGGL(flame::gaussian_kernel<false>, grid, block, 0, st, v, P, sigma, k0, k1, draw_stream, col0,
                       c_first, nblocks);
  return launch_status("add_gaussian");
}
