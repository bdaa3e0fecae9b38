// FoolsGold (Fung, Yoon, Beschastnikh, "The Limitations of Federated Learning in
// Sybil Settings", RAID 2020, Algorithm 1) on gfx950: the sybil defense.  Clients
// that resemble each other more than honest clients do lose their weight; the
// rule needs neither the attacker count nor a server dataset.
//
// The arithmetic is fixed (flr.h).  Four calls, each enqueued on the stream with
// no host synchronisation:
//   flr_rows_accumulate    H += X - center, the per-client history (HBM-bound:
//                          reads 2 * K * P * 4 bytes, writes K * P * 4)
//   flr_rows_gram          G = A A^T over all P coordinates, fp64, the products
//                          exact: v_mfma_f64_16x16x4_f64
//   flr_foolsgold_weights  one workgroup, a lane per client: cosines, pardoning,
//                          the logit, the normalised weights
//   flr_rows_combine_from  out = center + sum_i beta_i * (x_i - center), fp32, the
//                          rows with beta_i == 0 never read (flr_centered_clip's
//                          step without the division)
//
// The Gram kernel.  A workgroup of four waves owns one 64 x 64 block of G on or
// above the diagonal over one chunk of columns (a function of K and P: gram_chunks).
// It stages 64-column fp32 tiles of the two row blocks in LDS (one on a diagonal
// block), the next tile's global loads in flight while this one is summed; rows
// past K and columns past P enter as zeros through guarded loads.  Wave (wr, wc)
// holds the 2 x 2 MFMA accumulators of the 32 x 32 quarter at (32 wr, 32 wc).
// The f64 fragment: lane l = 16 q + r holds A[row r][k = q] and B[k = q][col r];
// D: col = l & 15, row = (l >> 4) + 4 * reg.  A lane reads 4 adjacent floats of
// its row at column 16 g + 4 q (one ds_read_b128; the 272-B row stride spreads a
// 16-lane group over all 64 banks) and feeds element s to MFMA s of the group:
// MFMA s of group g sums the columns 16 g + s + {0, 4, 8, 12}.  Both operands use
// that map, so every product pairs one column with itself; the order is fixed.
// The conversion fp32 -> fp64 happens between LDS and the fragment.  A wave whose
// quarter of a diagonal block lies below the diagonal issues no MFMA.
// One chunk: the block goes to G, every entry with i <= j also to its mirror.
// More: to the chunk's partial matrix; gram_reduce_kernel adds the partials in
// chunk order and writes G_ij and G_ji from the one sum (DnC's Gram, agg_dnc.hip,
// ends in the same kernel).  VEC (A, center 16-B aligned,
// lda % 4 == 0): float4 global loads; the same values reach the same LDS cells,
// so the same bits as the scalar path.
#include "rows_pass.h"

namespace flr {
namespace foolsgold {

using namespace rows;       // THREADS, STREAM (combine), the lane map, load / store (rows_pass.h)
constexpr int MAXK = 1024;  // the weights kernel: one lane per client
constexpr int COMBINE_MAXROWS = 4096;
constexpr int GB = 64;       // Gram: block edge, columns per LDS tile
constexpr int GLD = GB + 4;  // LDS row stride in floats (272 B)
constexpr int W_THREADS = 1024;
constexpr int W_WAVES = W_THREADS / 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- flr_rows_accumulate ----

// Row blockIdx.y; the lanes stride over the lane map (lane_columns).
template <bool VEC>
__global__ __launch_bounds__(THREADS) void accumulate_kernel(float* __restrict__ H, int64_t ldh,
                                                             const float* __restrict__ X, int64_t ldx,
                                                             const float* __restrict__ c, int64_t P) {
  float* h = H + (int64_t)blockIdx.y * ldh;
  const float* x = X + (int64_t)blockIdx.y * ldx;
  const int64_t lanes = VEC ? P / 4 + (P & 3) : P, stride = (int64_t)gridDim.x * THREADS;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < lanes; q += stride)
    lane_columns<VEC>(q, P, [&](auto w, int64_t p) {
      constexpr int W = decltype(w)::value;
      float hv[W], xv[W], cv[W];
      load<W>(h + p, hv);
      load<W>(x + p, xv);
      load<W>(c + p, cv);
#pragma unroll
      for (int e = 0; e < W; ++e) hv[e] = add_rn(hv[e], sub_rn(xv[e], cv[e]));
      store<W>(h + p, hv);
    });
}

// ---- flr_rows_gram ----

// The 64 x 64 blocks on or above the diagonal, and the column chunks they are
// summed over (ColumnChunks).
inline int gram_blocks(int64_t K) { return (int)((K + GB - 1) / GB); }
inline int gram_pairs(int64_t K) { return gram_blocks(K) * (gram_blocks(K) + 1) / 2; }
inline ColumnChunks gram_chunks(int64_t K, int64_t P) { return ColumnChunks(gram_pairs(K), P, GB); }

// One 64 x 64-column tile of row block r0 into registers: zeros past K and past
// pe; with a center, fl(a - center).
template <bool VEC>
__device__ __forceinline__ void gram_fetch(const float* __restrict__ A, int K, int64_t lda,
                                           const float* __restrict__ center, int r0, int64_t p0, int64_t pe,
                                           float (&v)[16]) {
  const int t = threadIdx.x;
  if constexpr (VEC) {
    const int64_t p = p0 + (t & 15) * 4;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (center) {
      if (p + 3 < pe) {
        const f32x4 cv = *reinterpret_cast<const f32x4*>(center + p);
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = cv[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p + e < pe) c[e] = center[p + e];
      }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int row = r0 + (t >> 4) + 16 * n;
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      bool in[4] = {false, false, false, false};
      if (row < K) {
        const float* src = A + (int64_t)row * lda + p;
        if (p + 3 < pe) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            x[e] = xv[e];
            in[e] = true;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (p + e < pe) {
              x[e] = src[e];
              in[e] = true;
            }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * n + e] = (center && in[e]) ? sub_rn(x[e], c[e]) : x[e];
    }
  } else {
    const int64_t p = p0 + (t & 63);
    const bool pin = p < pe;
    const float c = (center && pin) ? center[p] : 0.f;
#pragma unroll
    for (int n = 0; n < 16; ++n) {
      const int row = r0 + (t >> 6) + 4 * n;
      const bool in = pin && row < K;
      const float x = in ? A[(int64_t)row * lda + p] : 0.f;
      v[n] = (center && in) ? sub_rn(x, c) : x;
    }
  }
}

// The registers of gram_fetch into their cells of the LDS tile.
template <bool VEC>
__device__ __forceinline__ void gram_stage(float (*S)[GLD], const float (&v)[16]) {
  const int t = threadIdx.x;
  if constexpr (VEC) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = v[4 * n + e];
      *reinterpret_cast<f32x4*>(&S[(t >> 4) + 16 * n][(t & 15) * 4]) = o;
    }
  } else {
#pragma unroll
    for (int n = 0; n < 16; ++n) S[(t >> 6) + 4 * n][t & 63] = v[n];
  }
}

// Workgroup (x, y): block pair x (row block bi <= column block bj, the pairs in
// row-major order of the upper triangle), column chunk y.  mirror: dst is G
// itself (one chunk); otherwise dst + y * K * K is the chunk's partial matrix.
// The float4 form is held to 128 VGPRs (four workgroups per CU; measured faster
// than three); the 4-byte form would spill under that bound and is left alone.
template <bool VEC>
__global__ __launch_bounds__(THREADS, VEC ? 4 : 2) void gram_kernel(const float* __restrict__ A, int K, int64_t P, int64_t lda,
                                                       const float* __restrict__ center, int64_t chunk, int nb,
                                                       int mirror, double* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) float As[GB][GLD];
  __shared__ __attribute__((aligned(16))) float Bs[GB][GLD];
  int bi = 0, rest = blockIdx.x;
  while (rest >= nb - bi) {
    rest -= nb - bi;
    ++bi;
  }
  const int bj = bi + rest;
  const bool diag = bi == bj;
  const int i0 = bi * GB, j0 = bj * GB;
  const int64_t pb = (int64_t)blockIdx.y * chunk;
  const int64_t pe = pb + chunk < P ? pb + chunk : P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 15, q = lane >> 4;
  const bool work = !(diag && wr > wc);  // wave-uniform
  const float(*Bp)[GLD] = diag ? As : Bs;

  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

  float ra[16], rb[16];
  gram_fetch<VEC>(A, K, lda, center, i0, pb, pe, ra);
  if (!diag) gram_fetch<VEC>(A, K, lda, center, j0, pb, pe, rb);
  for (int64_t p0 = pb; p0 < pe; p0 += GB) {
    gram_stage<VEC>(As, ra);
    if (!diag) gram_stage<VEC>(Bs, rb);
    __syncthreads();
    if (p0 + GB < pe) {
      gram_fetch<VEC>(A, K, lda, center, i0, p0 + GB, pe, ra);
      if (!diag) gram_fetch<VEC>(A, K, lda, center, j0, p0 + GB, pe, rb);
    }
    if (work) {
#pragma unroll
      for (int g = 0; g < GB / 16; ++g) {
        const int col = 16 * g + 4 * q;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(&As[32 * wr + r][col]);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(&As[32 * wr + 16 + r][col]);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Bp[32 * wc + r][col]);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Bp[32 * wc + 16 + r][col]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double da0 = (double)a0[s], da1 = (double)a1[s], db0 = (double)b0[s], db1 = (double)b1[s];
          acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(da0, db0, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(da0, db1, acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(da1, db0, acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(da1, db1, acc[1][1], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (!work) return;
  double* out = dst + (mirror ? 0 : (int64_t)blockIdx.y * K * K);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + 32 * wr + 16 * a + q + 4 * reg;
        const int j = j0 + 32 * wc + 16 * b + r;
        if (i < K && j < K && i <= j) {
          out[(int64_t)i * K + j] = acc[a][b][reg];
          if (mirror) out[(int64_t)j * K + i] = acc[a][b][reg];
        }
      }
}

// G_ij = G_ji = the chunks' partial entries (i <= j) added in chunk order.
__global__ __launch_bounds__(THREADS) void gram_reduce_kernel(const double* __restrict__ part, int splits, int K,
                                                              double* __restrict__ G) {
  const int n = K * K;
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e >= n) return;
  const int i = e / K, j = e - i * K;
  if (i > j) return;
  double s = 0.0;
#pragma unroll 8
  for (int z = 0; z < splits; ++z) s += part[(int64_t)z * n + e];
  G[e] = s;
  G[(int64_t)j * K + i] = s;
}

// ---- flr_foolsgold_weights ----

// cs_ij from g = G_ji (G is symmetric: lane i's loads of column i coalesce).
__device__ __forceinline__ double cosine(double g, double ni, double nj, bool offdiag) {
  return (offdiag && ni > 0.0 && nj > 0.0) ? g / (ni * nj) : 0.0;
}

// One workgroup, lane t = client t.
__global__ __launch_bounds__(W_THREADS) void weights_kernel(const double* __restrict__ G, int K, double kappa,
                                                            double* __restrict__ alpha, float* __restrict__ beta,
                                                            double* __restrict__ maxcos_out,
                                                            int32_t* __restrict__ flags_out) {
  __shared__ double nrm[MAXK], vs[MAXK], al[MAXK], red[W_WAVES];
  __shared__ int ired[W_WAVES];
  const int t = threadIdx.x;
  const bool row = t < K;
  const double gtt = row ? G[(int64_t)t * K + t] : 0.0;
  const bool bad = row && !finite64(gtt);
  const bool good = row && !bad;
  const double nt = good ? sqrt(gtt) : 0.0;  // a bad row's 0 takes it out of every cosine
  nrm[t] = nt;
  __syncthreads();
  double v = 0.0;
  if (good) {
#pragma unroll 4
    for (int j = 0; j < K; ++j) {
      const double cs = cosine(G[(int64_t)j * K + t], nt, nrm[j], j != t);
      v = cs > v ? cs : v;
    }
  }
  vs[t] = v;
  __syncthreads();
  double mp = 0.0;
  if (good) {
#pragma unroll 4
    for (int j = 0; j < K; ++j) {
      const double cs = cosine(G[(int64_t)j * K + t], nt, nrm[j], j != t);
      const double vj = vs[j];
      const double pc = v < vj ? cs * v / vj : cs;
      mp = pc > mp ? pc : mp;
    }
  }
  double w = fmin(1.0, fmax(0.0, 1.0 - mp));
  const double top = block_reduce<W_WAVES>(good ? w : -1.0, red, [](double v, double o) { return o > v ? o : v; });
  const int anybad = block_reduce<W_WAVES>(bad ? 1 : 0, ired, [](int v, int o) { return v | o; });
  double a = 0.0;
  if (good && top > 0.0) {
    if (K == 1) {
      a = 1.0;
    } else {
      w = fmin(w / top, 0.99);
      a = fmin(1.0, fmax(0.0, kappa * (log(w / (1.0 - w)) + 0.5)));
    }
  }
  al[t] = row ? a : 0.0;
  __syncthreads();
  double S = 0.0;
  for (int i = 0; i < K; ++i) S += al[i];
  if (row) {
    alpha[t] = a;
    beta[t] = S > 0.0 ? (float)(a / S) : 0.f;
    if (maxcos_out) maxcos_out[t] = v;
  }
  if (t == 0 && flags_out) *flags_out = (S > 0.0 ? 0 : 1) | (anybad ? 2 : 0);
}

// ---- flr_rows_combine_from ----

// W adjacent coordinates from p on: the rows in groups of STREAM loads, each
// under its wave-uniform test of beta (a rejected row is not read); a partial
// last group tests the row index too.  Not stream_rows: its loads are unconditional.
template <int W>
__device__ __forceinline__ void combine_columns(const float* __restrict__ X, int K, int64_t ldx, int64_t p,
                                                const float* __restrict__ center, const float* bs,
                                                float* __restrict__ out) {
  float c[W], acc[W];
  load<W>(center + p, c);
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
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = add_rn(c[e], acc[e]);
  store<W>(out + p, acc);
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void combine_kernel(const float* __restrict__ X, int K, int64_t P, int64_t ldx,
                                                          const float* __restrict__ center,
                                                          const float* __restrict__ beta, float* __restrict__ out) {
  __shared__ float bs[COMBINE_MAXROWS];
  for (int t = threadIdx.x; t < K; t += THREADS) bs[t] = beta[t];
  __syncthreads();
  lane_columns<VEC>((int64_t)blockIdx.x * THREADS + threadIdx.x, P, [&](auto w, int64_t p) {
    combine_columns<decltype(w)::value>(X, K, ldx, p, center, bs, out);
  });
}

}  // namespace foolsgold

int rows::gram_reduce(const double* part, int splits, int K, double* G, hipStream_t st) {
  hipLaunchKernelGGL(foolsgold::gram_reduce_kernel, dim3((unsigned)((K * K + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                     st, part, splits, K, G);
  return launch_status("gram reduce");
}

}  // namespace flr

using namespace flr;

extern "C" int flr_rows_accumulate(float* H, int64_t ldh, const float* X, int64_t ldx, const float* center, int64_t K,
                                   int64_t P, void* stream) {
  if (!H || !X || !center || K < 1 || P < 1 || ldh < P || ldx < P || H == X) return FLR_ERR_ARG;
  if (K > 65535) return FLR_ERR_UNSUPPORTED;
  const bool vec = rows::vec_ok(H, X, center, ldh, ldx);
  int64_t nblocks = (rows::column_lanes(vec, P) + foolsgold::THREADS - 1) / foolsgold::THREADS;
  if (nblocks > 65536) nblocks = 65536;  // the lanes stride over the rest
  const dim3 grid((unsigned)nblocks, (unsigned)K), block(foolsgold::THREADS);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(foolsgold::accumulate_kernel<true>, grid, block, 0, st, H, ldh, X, ldx, center, P);
  else
    hipLaunchKernelGGL(foolsgold::accumulate_kernel<false>, grid, block, 0, st, H, ldh, X, ldx, center, P);
  return launch_status("rows_accumulate");
}

extern "C" int64_t flr_rows_gram_splits(int64_t K, int64_t P) {
  return (K < 1 || P < 1 || K > foolsgold::MAXK) ? 0 : foolsgold::gram_chunks(K, P).splits;
}

extern "C" size_t flr_rows_gram_workspace(int64_t K, int64_t P) {
  const int64_t splits = flr_rows_gram_splits(K, P);
  return splits > 1 ? align_up((size_t)splits * (size_t)K * (size_t)K * sizeof(double), 256) : 0;
}

extern "C" int flr_rows_gram(const float* A, int64_t K, int64_t P, int64_t lda, const float* center, double* G,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!A || !G || K < 1 || P < 1 || lda < P) return FLR_ERR_ARG;
  if (K > foolsgold::MAXK) return FLR_ERR_UNSUPPORTED;
  const rows::ColumnChunks plan = foolsgold::gram_chunks(K, P);
  if (plan.splits > 1 && (!workspace || workspace_bytes < flr_rows_gram_workspace(K, P) ||
                          (reinterpret_cast<uintptr_t>(workspace) & 255) != 0))
    return FLR_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const bool vec = rows::vec_ok(A, center, lda);
  const int mirror = plan.splits == 1 ? 1 : 0;
  double* dst = mirror ? G : static_cast<double*>(workspace);
  const dim3 grid((unsigned)foolsgold::gram_pairs(K), (unsigned)plan.splits), block(foolsgold::THREADS);
  if (vec)
    hipLaunchKernelGGL(foolsgold::gram_kernel<true>, grid, block, 0, st, A, (int)K, P, lda, center, plan.chunk,
                       foolsgold::gram_blocks(K), mirror, dst);
  else
    hipLaunchKernelGGL(foolsgold::gram_kernel<false>, grid, block, 0, st, A, (int)K, P, lda, center, plan.chunk,
                       foolsgold::gram_blocks(K), mirror, dst);
  int rc = launch_status("rows_gram");
  if (rc != FLR_OK || mirror) return rc;
  return rows::gram_reduce(static_cast<const double*>(workspace), plan.splits, (int)K, G, st);
}

extern "C" int flr_foolsgold_weights(const double* G, int64_t K, double kappa, double* alpha, float* beta,
                                     double* maxcos_out, int32_t* flags_out, void* stream) {
  if (!G || !alpha || !beta || K < 1 || !(kappa > 0.0) || !(kappa < __builtin_huge_val())) return FLR_ERR_ARG;
  if (K > foolsgold::MAXK) return FLR_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(foolsgold::weights_kernel, dim3(1), dim3(foolsgold::W_THREADS), 0, as_stream(stream), G, (int)K,
                     kappa, alpha, beta, maxcos_out, flags_out);
  return launch_status("foolsgold_weights");
}

extern "C" int flr_rows_combine_from(const float* X, int64_t K, int64_t P, int64_t ldx, const float* center,
                                     const float* beta, float* out, void* stream) {
  if (!X || !center || !beta || !out || K < 1 || P < 1 || ldx < P || out == center) return FLR_ERR_ARG;
  if (K > foolsgold::COMBINE_MAXROWS) return FLR_ERR_UNSUPPORTED;
  const bool vec = rows::vec_ok(X, center, out, ldx);
  const int64_t nblocks = (rows::column_lanes(vec, P) + foolsgold::THREADS - 1) / foolsgold::THREADS;
  if (nblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)nblocks), block(foolsgold::THREADS);
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(foolsgold::combine_kernel<true>, grid, block, 0, st, X, (int)K, P, ldx, center, beta, out);
  else
    hipLaunchKernelGGL(foolsgold::combine_kernel<false>, grid, block, 0, st, X, (int)K, P, ldx, center, beta, out);
  return launch_status("rows_combine_from");
}
