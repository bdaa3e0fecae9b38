// The column pass over a client matrix, shared by the aggregation and attack
// units (agg_mean, agg_norm, agg_cclip, agg_dnc, agg_flame, agg_foolsgold, agg_rlr,
// attack_colluding, attack_fang, attack_minmax, attack_replace): a lane owns one float4 of
// coordinates, or one coordinate, and walks the rows.  What is here has at least
// two users and takes no flag that says which caller it serves; a unit whose loop
// has another contract keeps it.
#pragma once

#include "flr_common.h"

#include <type_traits>

namespace flr {
namespace rows {

constexpr int THREADS = 256;  // the workgroup of grid_for and column_sum
constexpr int STREAM = 16;    // loads in flight per lane in stream_rows

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The value of lane 0 in an SGPR: tells the compiler it is wave-uniform.
__device__ __forceinline__ float uniform(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// W adjacent floats from / to p: W == 4 is one 16-B access (p 16-B aligned).
template <int W>
__device__ __forceinline__ void load(const float* __restrict__ p, float (&x)[W]) {
  if constexpr (W == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = t[e];
  } else {
    x[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void store(float* __restrict__ p, const float (&x)[W]) {
  if constexpr (W == 4) {
    f32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = x[e];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = x[0];
  }
}

// ---- the host side of the lane map ----

inline uintptr_t vec_bits(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }
inline uintptr_t vec_bits(int64_t ld) { return ld % 4 != 0; }

// The float4 lanes are usable: every pointer 16-B aligned (null counts as
// aligned) and every leading dimension a multiple of 4.
template <class... A>
inline bool vec_ok(A... ptrs_and_lds) {
  return (vec_bits(ptrs_and_lds) | ... | 0) == 0;
}

inline int64_t column_lanes(bool vec, int64_t P) { return vec ? P / 4 + (P & 3) : P; }

// The grid of a grid-stride pass: a workgroup per THREADS lanes, at most 256 x 16.
inline int grid_for(int64_t work) {
  int64_t g = (work + THREADS - 1) / THREADS;
  if (g > 256 * 16) g = 256 * 16;
  return (int)(g < 1 ? 1 : g);
}

// ---- the lane map ----

template <int W>
using width = std::integral_constant<int, W>;

// Lane q of column_lanes(VEC, P).  VEC: lane q < P / 4 owns coordinates
// [4q, 4q + 4), the next P % 4 lanes one coordinate of the tail each; otherwise
// lane q owns coordinate q.  f(width<W>{}, first coordinate), or nothing for a
// lane past the last.  A grid-stride kernel keeps its own loop over q around it.
template <bool VEC, class F>
__device__ __forceinline__ void lane_columns(int64_t q, int64_t P, F&& f) {
  if constexpr (VEC) {
    const int64_t nv = P / 4;
    if (q < nv) f(width<4>{}, 4 * q);
    else if (q < nv + (P & 3)) f(width<1>{}, 4 * nv + (q - nv));
  } else {
    if (q < P) f(width<1>{}, q);
  }
}

// ---- the row stream ----

// W adjacent coordinates from col on in the rows row_of(0 .. n-1), leading
// dimension ld: the rows in groups of STREAM loads, then use(k, x) in row order.
// The last, partial group re-reads the last row instead of testing each load (the
// loads issue back to back) and tests each use.
template <int W, class N, class R, class U>
__device__ __forceinline__ void stream_rows(const float* col, int64_t ld, N n, R&& row_of, U&& use) {
  const N nfull = n - n % STREAM;
  for (N k0 = 0; k0 < nfull; k0 += STREAM) {
    float t[STREAM][W];
#pragma unroll
    for (int i = 0; i < STREAM; ++i) load<W>(col + (int64_t)row_of(k0 + i) * ld, t[i]);
#pragma unroll
    for (int i = 0; i < STREAM; ++i) use(k0 + i, t[i]);
  }
  if (nfull < n) {
    float t[STREAM][W];
#pragma unroll
    for (int i = 0; i < STREAM; ++i) load<W>(col + (int64_t)row_of(nfull + i < n ? nfull + i : n - 1) * ld, t[i]);
#pragma unroll
    for (int i = 0; i < STREAM; ++i)
      if (nfull + i < n) use(nfull + i, t[i]);
  }
}

// ---- the plain column sum ----

// out = (sum over t < m, in order from +0, of term(t, X[row_of(t)])) / divisor for
// every coordinate: a grid-stride loop (grid_for) over float4 groups with the
// P % 4 tail on workgroup 0's first lanes, or over single coordinates.  skip(p):
// the float4 group at p is left unwritten.
template <bool VEC, class R, class T, class S>
__device__ __forceinline__ void column_sum(const float* __restrict__ X, int64_t P, int64_t ldx, int m, R&& row_of,
                                           T&& term, float divisor, float* __restrict__ out, S&& skip) {
  auto columns = [&](auto w, int64_t p) {
    constexpr int W = decltype(w)::value;
    float acc[W], x[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.f;
    for (int t = 0; t < m; ++t) {
      load<W>(X + (int64_t)row_of(t) * ldx + p, x);
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] = add_rn(acc[e], term(t, x[e]));
    }
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = div_rn(acc[e], divisor);
    store<W>(out + p, acc);
  };
  const int64_t first = (int64_t)blockIdx.x * THREADS + threadIdx.x, stride = (int64_t)gridDim.x * THREADS;
  if constexpr (VEC) {
    const int64_t nv = P / 4;
    for (int64_t q = first; q < nv; q += stride) {
      if (skip(4 * q)) continue;
      columns(width<4>{}, 4 * q);
    }
    if (blockIdx.x == 0 && threadIdx.x < (P & 3)) columns(width<1>{}, nv * 4 + threadIdx.x);  // scalar tail
  } else {
    for (int64_t p = first; p < P; p += stride) columns(width<1>{}, p);
  }
}
template <bool VEC, class R, class T>
__device__ __forceinline__ void column_sum(const float* __restrict__ X, int64_t P, int64_t ldx, int m, R&& row_of,
                                           T&& term, float divisor, float* __restrict__ out) {
  column_sum<VEC>(X, P, ldx, m, row_of, term, divisor, out, [](int64_t) { return false; });
}

// ---- one-workgroup reductions ----

// op over the WAVES * 64 lanes' v; every lane gets the same bits (the butterfly
// combines the same pairs in every lane, then each lane combines the wave results
// in wave order).  red: WAVES entries of LDS; the first barrier orders its reuse.
template <int WAVES, class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* red, Op&& op) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s = op(s, red[w]);
  return s;
}

// ---- the fp64 statistics' tests ----

__device__ __forceinline__ bool finite64(double x) {
  return ((uint64_t)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
// The larger / smaller value, a NaN once seen kept (numpy's max / min).
__device__ __forceinline__ double nanmax(double m, double v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ double nanmin(double m, double v) { return (v < m || v != v) ? v : m; }

// ---- the rank count ----

// Ascending order of the values as unsigned keys, NaN (either sign) last.
__device__ __forceinline__ uint32_t sort_key(float x) {
  if (x != x) return 0xffffffffu;
  const uint32_t u = __float_as_uint(x);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t sort_key(double x) {
  if (x != x) return 0xffffffffffffffffull;
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// Entry i's rank among the K keys: the keys below it, equal keys in index order.
// The ranks are a permutation of 0 .. K-1.
template <class Key>
__device__ __forceinline__ int rank_below(const Key* keys, int K, int i) {
  const Key ki = keys[i];
  int r = 0;
  for (int j = 0; j < K; ++j) {
    const Key kj = keys[j];
    r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
  }
  return r;
}

// ---- the Gram matrices' column chunks ----

// A K x K Gram matrix has few output tiles (DnC: 64 16 x 16 tiles at K = 128;
// FoolsGold: 3 64 x 64 blocks on or above the diagonal), so the columns are cut
// into chunks of whole LDS tiles, about 2048 workgroups in all (256 CUs x 4
// resident x 2) and at least 4 tiles each.  A function of the shape alone: the
// fp64 summation order is the same from run to run.
struct ColumnChunks {
  int64_t chunk;
  int splits;
  ColumnChunks(int64_t output_tiles, int64_t cols, int64_t tile_cols) {
    const int64_t want = 2048 / output_tiles;
    int64_t c = want < 1 ? cols : (cols + want - 1) / want;
    c = (c + tile_cols - 1) / tile_cols * tile_cols;
    if (c < 4 * tile_cols) c = 4 * tile_cols;
    chunk = c;
    splits = (int)((cols + c - 1) / c);
  }
};

// agg_foolsgold.hip: G_ij = G_ji = the chunks' K x K partial matrices' entries
// (i <= j) added in chunk order.  Both Gram kernels' partials are symmetric bit
// for bit (or hold the upper triangle only), so one sum serves both entries.
int gram_reduce(const double* part, int splits, int K, double* G, hipStream_t st);

}  // namespace rows
}  // namespace flr
