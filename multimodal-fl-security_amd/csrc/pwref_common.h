// Reference-exact Krum distances (agg_pairwise_ref*.hip): the constants, the
// tile numberings and the small host / device helpers every unit shares.  No
// inline asm here: the chain steps live in agg_pairwise_ref_dpp.hip and
// agg_pairwise_ref_quad.hip.  The design is in agg_pairwise_ref.hip's header.
#pragma once
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "flr_common.h"

namespace flr {
namespace pwref {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int IW = 4;              // I rows per wave: its 16-lane DPP rows
constexpr int JW = 16;             // J rows per wave: the lanes of a DPP row
constexpr int SB = 32;             // rows per super-block (tiles below)
constexpr int OFF_W = (SB / IW) * (SB / JW);  // waves of an off-diagonal super-block pair (16)
constexpr int DIAG_W = SB / IW;               // waves of a diagonal super-block (8)
constexpr int CS = 64;             // chain steps per staged chunk (256 B of one chain stream)
constexpr int NQ = CS / 4;         // 16-B pieces per chunk row
constexpr int RPD = 256 / CS;      // chunk rows per 1-KB DMA instruction (4)
constexpr int SROWS = 20;          // staged rows per stage (diagonal tiles read 19)
constexpr int NSTD = 4;            // ring stages of a dead region's mixed waves
constexpr int64_t XC_CAP = int64_t(8) << 30;  // bytes of one chain-major segment
constexpr int64_t XC_SLACK = 4096;            // bytes past the last stream the chunk prefetch may read
// A segment's streams are zero-filled from its last step up to a multiple of
// XC_GROUP steps (whole loop trips of every chain kernel: each asserts that its
// trip divides it): fma(0, 0, s) = s for the non-negative sums, so the loop
// runs whole groups without a per-chunk check and the last, partial chunk needs
// no separate path.
constexpr int64_t XC_GROUP = 8 * CS;
__host__ __device__ constexpr int64_t round_up_group(int64_t x) { return (x + XC_GROUP - 1) / XC_GROUP * XC_GROUP; }
static_assert(CS == 64 && NQ == 16, "x_i layout: 16 lanes x 4 steps per chunk");
// the XOR swizzle of a staged row's 16-B slots: the rows one ds_read_b128 lane
// group ({0-3,12-15,20-27}, {4-11,16-19,28-31} and +32) reads are distinct
// modulo 16, or the same row (a broadcast), on both tile kinds
__host__ __device__ constexpr int slot_swz(int row) { return row & 15; }

// Tiles (per chain): one wave each.  The K rows form super-blocks of 32;
// super-block pair (X, Y), X <= Y:
//  * X < Y: 32 x 32 pairs in OFF_W waves (g, h): I rows 32X + 4g + r (DPP row
//    r), J rows 32Y + 16h + lane % 16;
//  * X == Y: the super-block's 32 * 31 / 2 pairs as a circulant: I row a takes
//    J rows a + 1 .. a + 16 (mod 32), the antipodal pair (a, a + 16) once
//    (from a < 16); wave g holds a = 4g + r, so its J rows are 4g + 1 ..
//    4g + 19 (mod 32): 20 staged rows, lane (r, o - 1) reading row r + o - 1.
//    496 of 512 lanes hold a pair.
// Tiles are numbered Y-major: Y's tiles start at 8 Y^2; within Y the
// off-diagonal pairs X = 0 .. Y-1 (16 waves each, w = 2g + h), then the diagonal.
__host__ __device__ inline int tiles_before(int Y) { return DIAG_W * Y * Y; }
__host__ __device__ inline int ntiles_of(int K) { return tiles_before((K + SB - 1) / SB); }
struct Tile {
  int X, Y, g, h;
  bool diag;
};
__host__ __device__ inline Tile tile_of(int t) {
  int Y = 0;
  while (tiles_before(Y + 1) <= t) ++Y;  // at most ~K / 32 steps
  const int local = t - tiles_before(Y);
  Tile r;
  r.Y = Y;
  if (local < Y * OFF_W) {
    r.X = local / OFF_W;
    r.g = (local % OFF_W) >> 1;
    r.h = local & 1;
    r.diag = false;
  } else {
    r.X = Y;
    r.g = local - Y * OFF_W;
    r.h = 0;
    r.diag = true;
  }
  return r;
}
// the tile that computes pair (i, j), i < j
__host__ __device__ inline int tile_of_pair(int i, int j) {
  const int X = i / SB, Y = j / SB;
  if (X < Y) return tiles_before(Y) + X * OFF_W + 2 * ((i % SB) / IW) + (j % SB) / JW;
  const int a = i % SB, b = j % SB, o = b - a;  // 1 .. 31
  const int ii = o <= SB / 2 ? a : b;           // the row whose circulant half holds the pair
  return tiles_before(Y) + Y * OFF_W + ii / IW;
}
// A lane's pair (i, j) of tile T, the staged row it reads and whether it holds
// a pair at all (keep: a diagonal tile's antipodal pair once).  two: the
// two-chain tiles (tile2_of), I rows 8g + r and 8g + 4 + r — the second pair is
// (i + IW, j).
struct LanePair {
  int i, j, srow;
  bool keep;
};
__device__ __forceinline__ LanePair lane_pair(const Tile& T, int lane, bool two) {
  const int r = lane >> 4, jl = lane & 15;
  LanePair p;
  if (T.diag) {
    const int a = IW * T.g + r, o = jl + 1;
    p.i = SB * T.X + a;
    p.j = SB * T.X + ((a + o) & (SB - 1));
    p.srow = r + jl;
    p.keep = o < SB / 2 || a < SB / 2;
  } else {
    p.i = SB * T.X + (two ? 2 * IW : IW) * T.g + r;
    p.j = SB * T.Y + JW * T.h + jl;
    p.srow = jl;
    p.keep = true;
  }
  return p;
}

// Two chains per lane (ref_chain2_kernel): off-diagonal super-block pairs as 8
// waves of 8 I rows x 16 J rows, diagonal super-blocks as the circulant tiles
// above.  Tiles per Y: the off-diagonal pairs X = 0 .. Y-1 (8 waves each:
// w = 2g + h), then the diagonal.
__host__ __device__ inline int tiles2_before(int Y) { return 4 * Y * (Y + 1); }
__host__ __device__ inline int ntiles2_of(int K) { return tiles2_before((K + SB - 1) / SB); }
__host__ __device__ inline Tile tile2_of(int t) {
  int Y = 0;
  while (tiles2_before(Y + 1) <= t) ++Y;
  const int local = t - tiles2_before(Y);
  Tile r;
  r.Y = Y;
  if (local < 8 * Y) {
    r.X = local / 8;
    r.g = (local % 8) >> 1;
    r.h = local & 1;
    r.diag = false;
  } else {
    r.X = Y;
    r.g = local - 8 * Y;
    r.h = 0;
    r.diag = true;
  }
  return r;
}

// The throughput forms (agg_pairwise_ref_quad.hip): a wave holds ni I rows x 64
// J rows; the workgroup form groups 4 waves (32 I rows) of one J block.
constexpr int QJ = 64;   // J rows per wave (lanes)
constexpr int QTB = 16;  // transpose tile: rows x 4-step blocks
constexpr int QD = 8;    // x_j blocks in flight per lane
static_assert(XC_GROUP % (4 * QTB) == 0 && XC_GROUP % (4 * QD) == 0, "padded segments hold whole tiles / trips");
__host__ __device__ inline int64_t quad_rows(int64_t K) { return (K + QJ - 1) / QJ * QJ; }
// tiles of J block q (rows 64 q .. 64 q + 63): I blocks of ni rows a = 0 ..
// min(64 / ni (q + 1), ceil(K / ni)) - 1
__host__ __device__ inline int quad_ni(int q, int K, int ni) {
  const int a = QJ / ni * (q + 1), b = (K + ni - 1) / ni;
  return a < b ? a : b;
}
// bytes past a segment's last block the x_j / x_i prefetches may read
inline int64_t quad_slack(int64_t K) { return (QD + 4) * quad_rows(K) * 16; }
inline int quad_ntiles(int K, int ni) {
  int n = 0;
  for (int q = 0; q * QJ < K; ++q) n += quad_ni(q, K, ni);
  return n;
}
__host__ __device__ inline int wg_groups(int q, int K) { return (quad_ni(q, K, 8) + 3) / 4; }
inline int wg_ntiles(int K) {
  int n = 0;
  for (int q = 0; q * QJ < K; ++q) n += wg_groups(q, K);
  return n;
}
// Launch ordinal t -> (J block q, ordinal within it): the J blocks hold
// per_block(q, K) tiles each (quad_ni / wg_groups), numbered q-major.
struct QuadTile {
  int t, q;
};
template <class F>
__device__ __forceinline__ QuadTile find_tile(int t, int K, F per_block) {
  int q = 0;
  for (int n = per_block(0, K); t >= n; n = per_block(q, K)) {
    t -= n;
    ++q;
  }
  return {t, q};
}

constexpr int TW = 256;  // chain_transpose_kernel: steps per wave
// The transpose's waves to run, as runs of consecutive wave indices (wave w:
// steps w TW .. w TW + TW - 1): the host leaves out every wave whose 2048
// coordinates lie inside one tap-major block (tap_chain_kernel writes those),
// so no workgroup is launched only to find it has nothing to do.
struct WaveRuns {
  static constexpr int MAX = 48;
  int n;
  int64_t w0[MAX], pre[MAX + 1];  // run r: waves w0[r] .., launch ordinals pre[r] .. pre[r + 1] - 1
};

// A tap-major block of a training-order client matrix: a convolution weight
// stored [KK][Cin][Cout], KK = kh * kw, at columns off .. end() - 1 of every row,
// whose reference order is torch's [Cout][Cin][KK] (tap_chain_kernel).
constexpr int TAP_CO = 32;
constexpr int TAP_ROWS = 288;  // LDS tile rows (tap, input channel): CI = TAP_ROWS / KK
struct TapBlock {
  int64_t off, co, ci, kk;
  int64_t end() const { return off + co * ci * kk; }
  bool contains(int64_t u) const { return u >= off && u < end(); }
  int64_t tap_of(int64_t u) const { return (u - off) % kk; }
  // the stored column of reference coordinate u (tap_chain_kernel's loads are
  // the inverse: tile row (t, i), column o)
  int64_t column_of(int64_t u) const {
    const int64_t rel = u - off, o = rel / (ci * kk), i = (rel / kk) % ci, t = rel % kk;
    return off + (t * ci + i) * co + o;
  }
};
// The {off, Cout, Cin, KK} quadruples of the C API as blocks: ascending,
// disjoint, inside [0, limit), at most TAP_ROWS taps; false otherwise.
inline bool parse_taps(const int64_t* taps, int64_t ntaps, int64_t limit, std::vector<TapBlock>& out) {
  out.clear();
  int64_t end = 0;
  for (int64_t b = 0; b < ntaps; ++b) {
    const TapBlock t{taps[4 * b], taps[4 * b + 1], taps[4 * b + 2], taps[4 * b + 3]};
    if (t.off < end || t.off > limit || t.co < 1 || t.ci < 1 || t.kk < 1 || t.kk > TAP_ROWS || t.co > INT32_MAX ||
        t.ci > INT32_MAX || t.co > (limit - t.off) / (t.ci * t.kk))  // (no overflow: end() <= limit)
      return false;
    end = t.end();
    out.push_back(t);
  }
  return true;
}

// A dead-tap region (run_chain_regions): a 3 x 3 block at off % 8 == 0 whose dead
// taps every row shares (g, negated on rows < nneg).  Chain c's step s of the
// block (coordinate off + 8 s + c) has tap (c - s) mod 9, because 8 = -1
// (mod 9): the block's mask with period 9, at a phase that depends on the chain.
// Each chain is laid out on virtual steps v = s + 8 - c, so that every chain's
// period m = v / 9 visits the taps 8, 7, .. 0 in that order, and split into two
// streams: the live steps Xl[k][c][m NL + rank of the tap among the live ones]
// and the dead ones T[c][m ND + rank among the dead ones] = g + g, one row.
// The slots before a chain's first step and after its last are 0 in both
// streams: fma(0, 0, s) = s, the identity the padded chain streams rely on.
struct DeadPlan {
  int on;              // the compact form (tap_chain_kernel) / a dead region
  int nl, nd;          // live and dead taps
  uint64_t tap, rank;  // 4-bit fields: tap[n] = the n-th live tap, rank[t] = tap t's rank among its kind
};
__host__ __device__ inline int dead_nib(uint64_t v, int n) { return (int)((v >> (4 * n)) & 15); }
// slot of block coordinate rel (tap t) in its stream of n taps per period
__host__ __device__ inline int64_t dead_slot(int64_t rel, int t, int n, uint64_t rank) {
  const int64_t c = rel & 7, s = rel >> 3;
  return (s + 8 - c) / 9 * n + dead_nib(rank, t);
}

template <class F, int... U>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, U...>) {
  (f(std::integral_constant<int, U>{}), ...);
}

// the columns of the tail coordinates 8R .. P-1 (at most 7): ref_finish_kernel
struct TailCols {
  int64_t c[8];
};
// workspace layout: A [8][K][K] fp32 (256-B aligned), then the chain-major segment
inline size_t a_bytes(int64_t K) { return align_up((size_t)(8 * K * K) * 4, 256); }

}  // namespace pwref
}  // namespace flr
