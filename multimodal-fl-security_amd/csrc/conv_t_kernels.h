// The tiled GEMM kernels behind every tap-major convolution, the im2col / stem
// GEMMs and the batched GEMM: the shared epilogue, tgemm_kernel (fp32 LDS
// images: exact f32 and the pipelined bf16x6 loop), sgemm_kernel (split at
// stash), rgemm_kernel (the activation tile resident in LDS across the taps:
// layer1), wsgemm_kernel (transposed images: the weight gradient), rwgemm_kernel
// (the weight gradient with x and dy staged once for three taps: layer1),
// treduce_kernel (split-K).  conv_t_launch.h decides which of them a launch runs.
#pragma once

#include "conv_t_plans.h"

namespace flr {
namespace convt {

// XCD-aware tile order.  The hardware deals workgroups round-robin over the 8
// XCDs (linear id i -> XCD i % 8), each with its own 4 MB L2.  The remap gives
// XCD x one contiguous range of logical tiles (bijective for any grid size), so
// the tiles of one client — which re-read the same activations once per kernel
// tap and the same weight slabs once per pixel tile — run on one XCD and share
// its L2 instead of streaming every client through all eight.
__device__ __forceinline__ void xcd_tile(int& bx, int& by, int& bz) {
  const int gx = (int)gridDim.x, gy = (int)gridDim.y;
  const int n = gx * gy * (int)gridDim.z;
  const int lid = (int)blockIdx.x + gx * ((int)blockIdx.y + gy * (int)blockIdx.z);
  const int xcd = lid & 7, slot = lid >> 3;
  const int q = n >> 3, r = n & 7;
  const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  bx = t % gx;
  by = (t / gx) % gy;
  bz = t / (gx * gy);
}

template <class P> struct has_sq : std::false_type {};
template <bool V> struct has_sq<WgtT<V>> : std::true_type {};

// Sum over the workgroup in a fixed order (fp64): each thread's own value, a
// butterfly over the wave, the waves in index order; the result is thread 0's.
// Every thread of the workgroup must call it (one barrier).
__device__ __forceinline__ double block_sumsq(double s, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

// the epilogue's optional addend (DgradT: the other gradient path of a residual
// block, summed where autograd would add the two paths)
template <class P> __device__ inline const float* plan_add(const P&) { return nullptr; }
__device__ inline const float* plan_add(const DgradT& p) { return p.add; }

// ---- the epilogue ---------------------------------------------------------------
// Every GEMM kernel's: this wave's MSW x NS accumulator blocks (32 x 32 each) to
// the plan's output (S == 1: epilogue operands loaded before the stores) or to
// the split-K partials.  Block (i, j) lies in the tile at (m0 + off.m[i],
// n0 + off.n[j]), at (off.wr, off.wc) inside it; C/D map of the 32x32 MFMA:
// col = lane & 31 (l32), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (h).
template <int MSW, int NS>
struct TileOffs {
  int m[MSW], n[NS];  // the blocks' tiles: row / column offsets from (m0, n0)
  int wr, wc;         // the wave's block inside each tile (0: the tile is the block)
};
template <class Plan, int MSW, int NS>
__device__ __forceinline__ void store_tiles(const Plan& pl, int S, float* __restrict__ part, int k, int split, int m0,
                                            int n0, int h, int l32, int M, int N, f32x16 (&acc)[MSW][NS],
                                            const TileOffs<MSW, NS> off) {
#pragma unroll
  for (int i = 0; i < MSW; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int tm0 = m0 + off.m[i], tn0 = n0 + off.n[j];
      if (S == 1 && pl.linear()) {
        float* base = pl.out() + pl.tile_base(k, tm0, tn0);
        const int64_t ldm = pl.ldm();
        const int nl = off.wc + l32;
        if constexpr (std::is_base_of<BGemmArgs, Plan>::value) {
          if (pl.bias) {  // the batched GEMM's bias: one value per lane column, bias + v
            const float bv = tn0 + nl < N ? pl.bias[k * pl.bias_k + tn0 + nl] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = bv + acc[i][j][e];
          }
        }
        if (const float* abase = plan_add(pl)) {  // all 16 addends in flight before the first store
          abase += pl.tile_base(k, tm0, tn0);
          float av[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int ml = off.wr + (e & 3) + 8 * (e >> 2) + 4 * h;
            av[e] = (tm0 + ml < M && tn0 + nl < N) ? abase[ml * ldm + nl] : 0.f;
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = __fadd_rn(acc[i][j][e], av[e]);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int ml = off.wr + (e & 3) + 8 * (e >> 2) + 4 * h;
          if (tm0 + ml < M && tn0 + nl < N) base[ml * ldm + nl] = acc[i][j][e];
        }
        continue;
      }
      if constexpr (std::is_same<Plan, DgradT>::value) {
        if (S == 1 && pl.add) {  // parity-class stores: the addends loaded before any store
          int64_t ix[16];
          float av[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int m = tm0 + off.wr + (e & 3) + 8 * (e >> 2) + 4 * h;
            const int n = tn0 + off.wc + l32;
            ix[e] = (m < M && n < N) ? pl.index(k, m, n) : -1;
            av[e] = ix[e] >= 0 ? pl.add[ix[e]] : 0.f;
          }
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (ix[e] >= 0) pl.dx[ix[e]] = __fadd_rn(acc[i][j][e], av[e]);
          continue;
        }
      }
      if constexpr (std::is_base_of<BGemmArgs, Plan>::value) {
        if (S == 1) {
          pl.store_tile(k, tm0, tn0, off.wr + 4 * h, off.wc + l32, acc[i][j], M, N);
          continue;
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = tm0 + off.wr + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int n = tn0 + off.wc + l32;
        if (m < M && n < N) {
          if (S == 1) pl.store(k, m, n, acc[i][j][e]);
          else part[(((int64_t)split * pl.g.Kc + k) * M + m) * N + n] = acc[i][j][e];
        }
      }
    }
}

// wave (wm, wn)'s blocks in the 64 x 64 sub-tiles of a (64*MS) x (64*NS) workgroup tile
template <int MS, int NS>
__device__ __forceinline__ TileOffs<MS, NS> sub_tiles(int wm, int wn) {
  TileOffs<MS, NS> off;
#pragma unroll
  for (int i = 0; i < MS; ++i) off.m[i] = BM * i;
#pragma unroll
  for (int j = 0; j < NS; ++j) off.n[j] = BN * j;
  off.wr = 32 * wm;
  off.wc = 32 * wn;
  return off;
}

// The workgroup tile's clip-norm partial (WgtT with sq, S == 1; under split-K the
// treduce pass writes them): fp64, each thread's values in (i, j, e) order, then
// block_sumsq (red: the kernel's THREADS / 64 doubles of LDS); slot = the tile's
// index in the grid.  Every thread must call it.
template <class Plan, int MSW, int NS>
__device__ __forceinline__ void store_sumsq(const Plan& pl, int k, int bx, int by, int m0, int n0, int h, int l32, int M,
                                            int N, const f32x16 (&acc)[MSW][NS], const TileOffs<MSW, NS> off,
                                            double* red) {
  double sq = 0.0;
#pragma unroll
  for (int i = 0; i < MSW; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + off.m[i] + off.wr + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int n = n0 + off.n[j] + off.wc + l32;
        const double v = (m < M && n < N) ? (double)acc[i][j][e] : 0.0;
        sq += v * v;
      }
  const double t = block_sumsq(sq, red);
  if (threadIdx.x == 0) pl.sq[(int64_t)k * pl.sq_ld + by * (int)gridDim.x + bx] = t;
}

// ---- the kernel ---------------------------------------------------------------
// Workgroup tile (64*MS) x (64*NS): MS A sub-tiles and NS B sub-tiles of 64
// rows each are staged per K-tile; wave (wm, wn) owns rows 32 wm .. +31 and
// columns 32 wn .. +31 of every (i, j) sub-tile pair, so a fragment read from
// LDS feeds NS (A) or MS (B) MFMAs and the MS*NS accumulator chains are
// independent.  MS or NS = 2 halves the loads, LDS traffic and barriers per
// MFMA of the 64 x 64 tile.
template <class Plan, int MS, int NS, int X6>
__global__ __launch_bounds__(THREADS, 2) void tgemm_kernel(const Plan pl, int S, float* __restrict__ part, int remap,
                                                           int prio) {
  __shared__ __attribute__((aligned(16))) float As[2][MS][TILE];
  __shared__ __attribute__((aligned(16))) float Bs[2][NS][TILE];
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  const int k = bz / S, split = bz % S;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
  const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
  const int m0 = by * BM * MS, n0 = bx * BN * NS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;

  typename Plan::State sa[MS], sb[NS];
#pragma unroll
  for (int i = 0; i < MS; ++i) sa[i] = pl.init(k, m0 + BM * i, n0, tid);
#pragma unroll
  for (int j = 0; j < NS; ++j) sb[j] = pl.init(k, m0, n0 + BN * j, tid);
  float ra[MS][8], rb[NS][8];
  f32x16 acc[MS][NS];
#pragma unroll
  for (int i = 0; i < MS; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  auto load = [&](int r) {
#pragma unroll
    for (int i = 0; i < MS; ++i) pl.load_a(sa[i], r, ra[i]);
#pragma unroll
    for (int j = 0; j < NS; ++j) pl.load_b(sb[j], r, rb[j]);
  };
  auto stash_all = [&](int buf) {
#pragma unroll
    for (int i = 0; i < MS; ++i) stash<Plan::LA>(As[buf][i], ra[i], tid);
#pragma unroll
    for (int j = 0; j < NS; ++j) stash<Plan::LB>(Bs[buf][j], rb[j], tid);
  };
  // The six products over the MS x NS blocks, product-major (bf16x6.h's order: mfma6_product<P>).
  // The loops stay in the kernel body: inside a helper that takes the term arrays they compile to
  // another register allocation (profiles/gemm_core/README.md).
#define FLR_X6P(P, AH, AM, AL, BH, BM, BL)                                                        \
  _Pragma("unroll") for (int i = 0; i < MS; ++i) _Pragma("unroll") for (int j = 0; j < NS; ++j) \
      mfma6_product<P>(acc[i][j], AH[i], AM[i], AL[i], BH[j], BM[j], BL[j]);
#define FLR_X6P_ALL(...)                                                                           \
  FLR_X6P(0, __VA_ARGS__) FLR_X6P(1, __VA_ARGS__) FLR_X6P(2, __VA_ARGS__) FLR_X6P(3, __VA_ARGS__) \
  FLR_X6P(4, __VA_ARGS__) FLR_X6P(5, __VA_ARGS__)
  if constexpr (X6 == 2) {
    // Software-pipelined bf16x6 loop (the default form).  A wave issues in
    // order, so its fragment reads, bf16 splits, LDS stash and global loads
    // only overlap its own MFMAs when they sit between them in one basic
    // block.  Per K-tile t (two 16-deep k-steps, fragments F of step 0 ready):
    //   phase 0: MFMAs of step 0 || read + split step 1 -> F1, stash tile t+1
    //   barrier (publishes tile t+1; every read of the buffer it reuses is done)
    //   phase 1: MFMAs of step 1 || global loads of tile t+2, read + split
    //            step 0 of tile t+1 -> F0
    // Tiles past the last are clamped to it (duplicate loads / stashes / splits
    // that nothing consumes), so both phases are branch-free.
    static_assert(BK == 32, "two k-steps per K-tile");
    const int ntile = rend > rbeg ? (rend - rbeg + BK - 1) / BK : 0;
    if (ntile > 0) {
      const int rlast = rbeg + (ntile - 1) * BK;
      bf16x8 ah0[MS], am0[MS], al0[MS], bh0[NS], bm0[NS], bl0[NS];
      bf16x8 ah1[MS], am1[MS], al1[MS], bh1[NS], bm1[NS], bl1[NS];
      float va[MS][8], vb[NS][8];
      auto read_frags = [&](int buf, int s) {
#pragma unroll
        for (int i = 0; i < MS; ++i) frag8<Plan::LA>(As[buf][i], 32 * wm + l32, 16 * s + 8 * h, va[i]);
#pragma unroll
        for (int j = 0; j < NS; ++j) frag8<Plan::LB>(Bs[buf][j], 32 * wn + l32, 16 * s + 8 * h, vb[j]);
      };
#define FLR_SPLIT_ALL(AH, AM, AL, BH, BM, BL)                                       \
  _Pragma("unroll") for (int i = 0; i < MS; ++i) split3_dot2(va[i], AH[i], AM[i], AL[i]); \
  _Pragma("unroll") for (int j = 0; j < NS; ++j) split3_dot2(vb[j], BH[j], BM[j], BL[j]);
      load(rbeg);
      stash_all(0);
      __syncthreads();
      load(std::min(rbeg + BK, rlast));
      read_frags(0, 0);
      FLR_SPLIT_ALL(ah0, am0, al0, bh0, bm0, bl0)
      int cur = 0;
      for (int t = 0; t < ntile; ++t) {
        const int r0 = rbeg + t * BK;
        // phase 0
        read_frags(cur, 1);
        FLR_X6P_ALL(ah0, am0, al0, bh0, bm0, bl0)
        FLR_SPLIT_ALL(ah1, am1, al1, bh1, bm1, bl1)
        stash_all(cur ^ 1);
        __syncthreads();
        // phase 1
        load(std::min(r0 + 2 * BK, rlast));
        read_frags(cur ^ 1, 0);
        FLR_X6P_ALL(ah1, am1, al1, bh1, bm1, bl1)
        FLR_SPLIT_ALL(ah0, am0, al0, bh0, bm0, bl0)
        cur ^= 1;
      }
#undef FLR_SPLIT_ALL
    }
  } else {
  if (rbeg < rend) {
    load(rbeg);
    stash_all(0);
  }
  __syncthreads();
  int cur = 0;
  for (int r0 = rbeg; r0 < rend; r0 += BK) {
    const bool more = r0 + BK < rend;
    if (more) load(r0 + BK);  // in flight during the MFMAs below
    if constexpr (X6 != 0) {
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        bf16x8 ah[MS], am[MS], al[MS], bh[NS], bm[NS], bl[NS];
#pragma unroll
        for (int i = 0; i < MS; ++i) {
          float v[8];
          frag8<Plan::LA>(As[cur][i], 32 * wm + l32, 16 * s + 8 * h, v);
          if constexpr (X6 == 3) {
#pragma unroll
            for (int q = 0; q < 8; ++q) ah[i][q] = am[i][q] = al[i][q] = (__bf16)v[q];
          } else {
            split3_dot2(v, ah[i], am[i], al[i]);
          }
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          float v[8];
          frag8<Plan::LB>(Bs[cur][j], 32 * wn + l32, 16 * s + 8 * h, v);
          if constexpr (X6 == 3) {
#pragma unroll
            for (int q = 0; q < 8; ++q) bh[j][q] = bm[j][q] = bl[j][q] = (__bf16)v[q];
          } else {
            split3_dot2(v, bh[j], bm[j], bl[j]);
          }
        }
        if (prio) __builtin_amdgcn_s_setprio(1);
        if constexpr (X6 >= 3) {
          FLR_X6P_ALL(ah, am, al, bh, bm, bl)
        } else {  // accumulator-chain order: each block's six products back to back
#pragma unroll
          for (int i = 0; i < MS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) acc[i][j] = mfma6(acc[i][j], ah[i], am[i], al[i], bh[j], bm[j], bl[j]);
        }
        if (prio) __builtin_amdgcn_s_setprio(0);
      }
    } else {
      f32x4 fa[MS][4], fb[NS][4];  // all of the tile's fragments first: the reads overlap the MFMA chain
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
        for (int i = 0; i < MS; ++i) fa[i][jj] = frag<Plan::LA>(As[cur][i], 32 * wm + l32, jj, h);
#pragma unroll
        for (int j = 0; j < NS; ++j) fb[j][jj] = frag<Plan::LB>(Bs[cur][j], 32 * wn + l32, jj, h);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of the chain (the scheduler would interleave them)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < MS; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][jj][t], fb[j][jj][t], acc[i][j], 0, 0, 0);
    }
    if (more) stash_all(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  }  // old loop (FLR_GEMM=f32 | chain | old | A)
#undef FLR_X6P_ALL
#undef FLR_X6P
  const TileOffs<MS, NS> off = sub_tiles<MS, NS>(wm, wn);
  store_tiles<Plan, MS, NS>(pl, S, part, k, split, m0, n0, h, l32, M, N, acc, off);
  if constexpr (has_sq<Plan>::value) {
    if (S == 1 && pl.sq) {
      __shared__ double red[THREADS / 64];
      store_sumsq(pl, k, bx, by, m0, n0, h, l32, M, N, acc, off, red);
    }
  }
}

// ---- the split-at-stash form (FLR_GEMM=stash) ------------------------------
// Each value is split into bf16 hi/mid/lo ONCE, by the thread that loaded it,
// instead of once per wave that reads its fragment: the LDS holds three bf16
// images per sub-tile, [64 rows][32 k] with the four 16-B k-chunks of a row
// XOR-swizzled by zswz(row) (no padding: conflict-free ds_read_b128 fragment
// reads and ds_write_b128 stashes under both stash mappings, checked
// exhaustively over the lane groups), and an MFMA fragment is one
// ds_read_b128 per term.  48 KB per 128 x 128 tile, so three workgroups fit a
// CU's LDS (the padded 80-B rows took 61 KB: two).  The loads are k-contiguous (thread: row tid & 63,
// k 8 (tid >> 6) .. +7, the plans' init8 / load_a8 / load_b8), so a thread's
// stash is three 16-B writes per sub-tile.  Single LDS buffer, two barriers
// per K-tile; the split of tile t+1 sits between tile t's MFMAs.  Every
// accumulator sees the same bf16 products in the same order as the other
// bf16x6 forms: the results are bit-identical to them.
constexpr int SB = 32;            // bf16 per image row (chunks swizzled, no pad)
constexpr int TERM_B = 64 * SB;   // bf16 per term image
// bf16 offset of (row, k-chunk c = k / 8) in a row-major term image
__device__ __forceinline__ int zimg(int row, int c) {
  const int f = ((row >> 2) & 1) | ((((row >> 1) ^ (row >> 3)) & 1) << 1);
  return row * SB + 8 * (c ^ f);
}
// waves per SIMD the split-at-stash kernels are compiled for (3 would mean at
// most 168 VGPRs, three 128 x 128 workgroups per CU)
constexpr int SG_OCC = 2;
template <class P> struct has_k8 : std::false_type {};
template <> struct has_k8<FwdT> : std::true_type {};
template <> struct has_k8<DgradT> : std::true_type {};
// WgtT has k8 loads but stays on the pipelined form: its x operand is k-contiguous
// only along pixels, so the k8 mapping puts the lanes on channels (sxc apart, a
// cache line per lane): l1 wgrad 202 -> 366 us measured.
template <int A, int B> struct has_k8<BGemm<A, B>> : std::true_type {};
// Two LDS stages (one barrier per K-tile, tile t+1 stashed into the other stage
// during tile t's MFMAs, one workgroup per CU by LDS) were measured 20-35 %
// slower than this one-stage form at two workgroups per CU (C3 conv and C4
// GEMM shapes, profiles/r3_sgemm_db.txt).
//
// Producer / consumer waves (8 consumer waves over a 128 x 256 tile + 4 waves that
// only stash into the other of two LDS stages, one barrier per K-tile; or 4 + 4 over
// 128 x 128) were measured, bit-identical, 7-40 % slower than this loop on the C4
// GEMM and C3 conv shapes (profiles/r3_gemm_loop/pc8_*): the consumer waves, which
// wait for their fragment reads after every barrier, set the pace.
//
// A half-phase schedule (one barrier per 16-deep k-step; waves 0-1 stash k-step 0's
// half of the next tile beside k-step 1's MFMAs, waves 2-3 k-step 1's half beside
// the next k-step 0; lane pairs instead of quads on k-contiguous rows) was
// bit-identical and 0-25 % slower per conv layer, 8-27 % on the C4 GEMMs, C3 round
// 60.0 -> 61.5 ms (profiles/r3_gemm_loop/half_phase.txt): twice the barriers per MFMA.
// Issuing tile t+2's global loads before the first barrier instead of after the
// stash: neutral on the GEMMs, C3 round 58.7 -> 59.6 ms (same file).
// NAR (narrow N, the l4 convolutions' N = B * 1 * 1 = 32 pixels): NS = 1 and the four
// waves stacked along M over MS 64-row A sub-tiles, each wave MS / 2 MFMA blocks of
// 32 x 32 on the first 32 columns of the B image — a 64-wide N tile would leave half
// its MFMAs on empty columns.  Same products per output: bit-identical.
template <class Plan, int MS, int NS, int ABL = 0, bool NAR = false>
__device__ __forceinline__ void sgemm_body(const Plan& pl, int S, float* __restrict__ part, int remap) {
  static_assert(!NAR || (NS == 1 && (MS == 2 || MS == 4)), "narrow tiles: 128 or 256 x 32");
  constexpr int MSW = NAR ? MS / 2 : MS;  // MFMA blocks per wave along M (NAR), or A sub-tiles
  __shared__ __attribute__((aligned(16))) __bf16 Ls[MS + NS][3][TERM_B];
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  if (remap >> 8) odd_slot_controls(remap);
  const int k = bz / S, split = bz % S;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
  const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
  const int m0 = by * BM * MS, n0 = bx * BN * NS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  // this thread's stash row and k offset per operand (Plan::QUAD_A / QUAD_B)
  const int srowA = stash_row<Plan::QUAD_A>(tid), skA = stash_k<Plan::QUAD_A>(tid);
  const int srowB = stash_row<Plan::QUAD_B>(tid), skB = stash_k<Plan::QUAD_B>(tid);

  typename Plan::State8 sa[MS], sb[NS];
#pragma unroll
  for (int i = 0; i < MS; ++i) sa[i] = pl.init8(k, m0 + BM * i, n0, tid);
#pragma unroll
  for (int j = 0; j < NS; ++j) sb[j] = pl.init8(k, m0, n0 + BN * j, tid);
  // one register set: a second one, keeping two tiles of global loads in flight, was measured: no gain
  // at the C3 conv and C4 GEMM shapes — the loop is not load-latency-bound
  float ra[MS][8], rb[NS][8];
  bf16x8 pa[MS][3], pb[NS][3];
  f32x16 acc[MSW][NS];
#pragma unroll
  for (int i = 0; i < MSW; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // this wave's MFMA block i: A sub-tile and row band (NAR: wave-stacked), and its
  // row / column offset from (m0, n0)
  auto a_sub = [&](int i) { return NAR ? (wave * MSW + i) >> 1 : i; };
  auto a_row = [&](int i) { return NAR ? 32 * ((wave * MSW + i) & 1) + l32 : 32 * wm + l32; };
  auto b_row = [&]() { return NAR ? l32 : 32 * wn + l32; };
  auto m_off = [&](int i) { return NAR ? 32 * (wave * MSW + i) : BM * i + 32 * wm; };
  auto n_off = [&](int j) { return NAR ? 0 : BN * j + 32 * wn; };
  auto load = [&](int r) {
#pragma unroll
    for (int i = 0; i < MS; ++i) pl.load_a8(sa[i], r, ra[i]);
#pragma unroll
    for (int j = 0; j < NS; ++j) pl.load_b8(sb[j], r, rb[j]);
  };
  auto split_all = [&]() {
#pragma unroll
    for (int i = 0; i < MS; ++i) split3_dot2(ra[i], pa[i][0], pa[i][1], pa[i][2]);
#pragma unroll
    for (int j = 0; j < NS; ++j) split3_dot2(rb[j], pb[j][0], pb[j][1], pb[j][2]);
  };
  auto write_all = [&]() {
#pragma unroll
    for (int i = 0; i < MS; ++i)
#pragma unroll
      for (int t = 0; t < 3; ++t) *reinterpret_cast<bf16x8*>(&Ls[i][t][zimg(srowA, skA >> 3)]) = pa[i][t];
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int t = 0; t < 3; ++t) *reinterpret_cast<bf16x8*>(&Ls[MS + j][t][zimg(srowB, skB >> 3)]) = pb[j][t];
  };
  // Both k-steps' fragments are read before the first MFMA, so the second
  // k-step's LDS latency runs under the first's MFMAs and the reads are complete
  // by the barrier that follows (the compiler keeps the reads ahead of that
  // barrier and moves the second k-step's MFMAs after it).  Reading per k-step
  // (same operands, same MFMA order) was the A/B: profiles/r6_conv/README.md.
  auto compute_tile = [&]() {
    constexpr int NKS = BK / 16;
    bf16x8 fa[NKS][MSW][3], fb[NKS][NS][3];
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      const int ko = 16 * s + 8 * h;
#pragma unroll
      for (int i = 0; i < MSW; ++i)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          fa[s][i][q] = *reinterpret_cast<const bf16x8*>(&Ls[a_sub(i)][q][zimg(a_row(i), ko >> 3)]);
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          fb[s][j][q] = *reinterpret_cast<const bf16x8*>(&Ls[MS + j][q][zimg(b_row(), ko >> 3)]);
    }
    __builtin_amdgcn_sched_barrier(0);  // the scheduler would sink the second k-step's reads again
#pragma unroll
    for (int s = 0; s < NKS; ++s) mfma6_blocks<MSW, NS>(acc, fa[s], fb[s]);
  };
  const int ntile = rend > rbeg ? (rend - rbeg + BK - 1) / BK : 0;
  if (ntile > 0) {
    const int rlast = rbeg + (ntile - 1) * BK;
    load(rbeg);
    split_all();
    write_all();
    load(std::min(rbeg + BK, rlast));
    __syncthreads();
    // one K-tile: the MFMAs of tile t from the LDS images, the split of tile t+1
    // between them, its stash, then the global loads of tile t+2 into the
    // registers just freed (clamped past the last tile: duplicates)
    auto tile_body = [&](int t) {
      const int r0 = rbeg + t * BK;
      // ABL (tools build only, timing ablations with wrong results): 1 no global loads,
      // 2 no stash writes, 4 no first barrier, 8 no split, 16 no MFMAs / fragment reads
      // (profiles/r3_gemm_loop/: without the stash writes the loop is 36 % shorter; with
      // only the fragment reads and MFMAs it runs at ~0.55 of the bf16x6 ceiling)
      if constexpr (!(ABL & 16)) compute_tile();
      if constexpr (!(ABL & 8)) split_all();
      if constexpr (!(ABL & 4)) __syncthreads();  // every wave's fragment reads of tile t are done
      if constexpr (!(ABL & 2)) write_all();
      if constexpr (!(ABL & 1)) load(std::min(r0 + 2 * BK, rlast));
      __syncthreads();
    };
    for (int t = 0; t < ntile; ++t) tile_body(t);
  }
  TileOffs<MSW, NS> off;
#pragma unroll
  for (int i = 0; i < MSW; ++i) off.m[i] = m_off(i);
#pragma unroll
  for (int j = 0; j < NS; ++j) off.n[j] = n_off(j);
  off.wr = off.wc = 0;
  store_tiles<Plan, MSW, NS>(pl, S, part, k, split, m0, n0, h, l32, M, N, acc, off);
}

template <class Plan, int MS, int NS, int ABL = 0, bool NAR = false>
__global__ __launch_bounds__(THREADS, SG_OCC) void sgemm_kernel(const Plan pl, int S, float* __restrict__ part,
                                                                 int remap) {
  sgemm_body<Plan, MS, NS, ABL, NAR>(pl, S, part, remap);
}

// ---- the resident-B form (layer1's forward and stride-1 data gradient) ----------
// A stride-1 "same" convolution reads the SAME reduction channels x pixels at every
// tap, only shifted by (dh, dw): sgemm_body gathers, splits and stashes that operand
// once per tap.  Here the workgroup tile is 64 (M) x 128 (N) with the 128 columns
// whole images (128 / (H W) of them) and the reduction channels are 64, so the raw B
// operand of the tile — 64 channels x 128 pixels — is split once, in the prologue,
// into bf16 term images that stay in LDS: one per 32-channel chunk and term,
// [129 rows][32 k] with zimg's swizzle, row = pixel index in the tile, row 128 zeros
// (columns past N are zero rows too).  Per K-tile only the 64 x 32 weight sub-tile
// goes through load -> split -> stash; the B fragment of lane column n at the
// K-tile's tap is one ds_read_b128 per term at the row of the shifted pixel of the
// same image, or row 128 where the tap reads padding (load_b8's predicate, once per
// tap).  K-tile order, k-steps and the six products per accumulator are
// sgemm_body's, a padding position contributes the same zero operand: bit-identical.
// Split-K 1 only (resident_ok).  LDS: 12,288 B (A) + 49,536 B (B) = 61,824 B, two
// workgroups per CU.
constexpr int RES_N = 128;                 // columns of the tile: whole images
constexpr int RES_IMG = (RES_N + 1) * SB;  // bf16 per resident term image (row 128: zeros)

template <class Plan>
__global__ __launch_bounds__(THREADS, SG_OCC) void rgemm_kernel(const Plan pl, int remap) {
  __shared__ __attribute__((aligned(16))) __bf16 La[3][TERM_B];
  __shared__ __attribute__((aligned(16))) __bf16 Lb[2][3][RES_IMG];
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  if (remap >> 8) odd_slot_controls(remap);
  const int k = bz;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int m0 = by * BM, n0 = bx * RES_N;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  const int srowA = stash_row<Plan::QUAD_A>(tid), skA = stash_k<Plan::QUAD_A>(tid);
  const int Hh = pl.g.H, Ww = pl.g.W;

  const typename Plan::State8 sa = pl.init8(k, m0, n0, tid);
  float ra[8];
  bf16x8 pa[3];
  f32x16 acc[1][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[0][j][e] = 0.f;
  auto write_a = [&]() {
#pragma unroll
    for (int t = 0; t < 3; ++t) *reinterpret_cast<bf16x8*>(&La[t][zimg(srowA, skA >> 3)]) = pa[t];
  };
  const int rlast = R - BK;  // R = taps x 64: at least two K-tiles
  pl.load_a8(sa, 0, ra);
  {  // the resident image: thread (pixel row 64 j + tid % 64, channels 32 c + 8 (tid / 64) .. +7)
    const rsrc_t rb = pl.res_rsrc(k);
    const int cs = pl.res_cs(), kc = tid >> 6;
    float rbv[2][2][8];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + 64 * j + (tid & 63);
      int oh, ow;
      const int off = pl.res_col(n, oh, ow);
      const unsigned vb = n < N ? (unsigned)((off + 8 * kc * cs) * 4) : SENT;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) rbv[j][c][e] = ld1(rb, vb, (32 * c + e) * cs * 4);
    }
    split3_dot2(ra, pa[0], pa[1], pa[2]);
    write_a();
    pl.load_a8(sa, std::min(BK, rlast), ra);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        bf16x8 pb[3];
        split3_dot2(rbv[j][c], pb[0], pb[1], pb[2]);
#pragma unroll
        for (int t = 0; t < 3; ++t)
          *reinterpret_cast<bf16x8*>(&Lb[c][t][zimg(64 * j + (tid & 63), kc)]) = pb[t];
      }
    if (tid < 24) {  // the zero row of the six images: four 16-B chunks each
      bf16x8 z;
#pragma unroll
      for (int q = 0; q < 8; ++q) z[q] = (__bf16)0.f;
      *reinterpret_cast<bf16x8*>(&Lb[0][0][0] + (tid >> 2) * RES_IMG + RES_N * SB + 8 * (tid & 3)) = z;
    }
  }
  // this lane's two columns: tile row and pixel
  int crow[2], coh[2], cow[2], brow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    crow[j] = BN * j + 32 * wn + l32;
    pl.res_col(n0 + crow[j], coh[j], cow[j]);
  }
  __syncthreads();
  // one K-tile (channel chunk C of the tap whose rows are brow): both k-steps'
  // fragments before the first MFMA, the split of the next A sub-tile between the
  // MFMAs, its stash, then the global loads of the one after (clamped: duplicates)
  auto tile_body = [&](int t, auto C) {
    constexpr int c = decltype(C)::value;
    constexpr int NKS = BK / 16;
    bf16x8 fa[NKS][1][3], fb[NKS][2][3];
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        fa[s][0][q] = *reinterpret_cast<const bf16x8*>(&La[q][zimg(32 * wm + l32, 2 * s + h)]);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          fb[s][j][q] = *reinterpret_cast<const bf16x8*>(&Lb[c][q][zimg(brow[j], 2 * s + h)]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < NKS; ++s) mfma6_blocks<1, 2>(acc, fa[s], fb[s]);
    split3_dot2(ra, pa[0], pa[1], pa[2]);
    __syncthreads();  // every wave's fragment reads of tile t are done
    write_a();
    pl.load_a8(sa, std::min((t + 2) * BK, rlast), ra);
    __syncthreads();
  };
  const int nslot = R / (2 * BK);
  for (int slot = 0; slot < nslot; ++slot) {
    int dh, dw;
    pl.res_shift(slot, dh, dw);
    dh = uni(dh);
    dw = uni(dw);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ih = coh[j] + dh, iw = cow[j] + dw;
      const bool ok = (ih >= 0) & (ih < Hh) & (iw >= 0) & (iw < Ww);
      brow[j] = ok ? crow[j] + dh * Ww + dw : RES_N;
    }
    tile_body(2 * slot, std::integral_constant<int, 0>());
    tile_body(2 * slot + 1, std::integral_constant<int, 1>());
  }
  TileOffs<1, 2> off;
  off.m[0] = 32 * wm;
#pragma unroll
  for (int j = 0; j < 2; ++j) off.n[j] = BN * j + 32 * wn;
  off.wr = off.wc = 0;
  store_tiles<Plan, 1, 2>(pl, 1, nullptr, k, 0, m0, n0, h, l32, M, N, acc, off);
}

// ---- the weight gradient on split-at-stash images, transposed ----------------
// Both operands of dW are contiguous along the reduction (pixels), so the loads
// put a half-wave on 32 consecutive pixels of one channel (coalesced) and each
// thread holds 8 consecutive channels at one pixel (StateT).  The split images
// are [k = 32][row = 64] bf16 per term (128-B k-rows, 16-B chunks of 8 rows
// XOR-swizzled by tswz(k): conflict-free ds_write_b128 stashes and transposed
// reads), and an MFMA fragment (8 consecutive k of one row) is two
// ds_read_b64_tr_b16: each 16-lane group reads a 4 k x 16 row block and gets it
// column-major.  Products and their order per accumulator are the other bf16x6
// forms': bit-identical dw and clip-norm partials.
typedef short s16x4 __attribute__((ext_vector_type(4)));
__host__ __device__ constexpr int tswz(int k) { return (k & 3) | ((((k >> 1) ^ (k >> 2)) & 1) << 2); }
constexpr int TIMG = 32 * 64;  // bf16 per transposed term image

template <class Plan, int MS, int NS, bool TA, bool TB>
__global__ __launch_bounds__(THREADS, SG_OCC) void wsgemm_kernel(const Plan pl, int S, float* __restrict__ part,
                                                                  int remap) {
  // a term image: transposed [32 k][64 rows] (TIMG) or row-major [64 rows][SB] (TERM_B)
  constexpr int IMG = (TA || TB) && !(TA && TB) ? TERM_B : (TA ? TIMG : TERM_B);
  __shared__ __attribute__((aligned(16))) __bf16 Lt[MS + NS][3][IMG];
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  if (remap >> 8) odd_slot_controls(remap);
  const int k = bz / S, split = bz % S;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
  const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
  const int m0 = by * BM * MS, n0 = bx * BN * NS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  // stash slot: k = tid & 31, chunk (tid >> 5) ^ tswz(k)
  const int skq = tid & 31;
  const int sidx = skq * 64 + 8 * ((tid >> 5) ^ tswz(skq));
  // transposed-read lane addresses (bf16 index in a term image) for the two 4-k halves
  // of this lane's 8-k fragment; k-step s adds 16 * 64
  const int gq = (lane & 15) >> 2, gp = lane & 3, g1 = (lane >> 4) & 1;
  int ra_off[2], rb_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kk = 8 * h + 4 * j + gq;
    const int ca = 4 * wm + 2 * g1 + (gp >> 1), cb = 4 * wn + 2 * g1 + (gp >> 1);
    ra_off[j] = kk * 64 + 8 * (ca ^ tswz(kk)) + 4 * (gp & 1);
    rb_off[j] = kk * 64 + 8 * (cb ^ tswz(kk)) + 4 * (gp & 1);
  }

  // row-major images: the split-at-stash kernel's stash slot and fragment rows
  const int srowA = stash_row<Plan::QUAD_A>(tid), skA = stash_k<Plan::QUAD_A>(tid);
  const int srowB = stash_row<Plan::QUAD_B>(tid), skB = stash_k<Plan::QUAD_B>(tid);
  using SA = std::conditional_t<TA, typename Plan::StateT, typename Plan::State8>;
  using SBt = std::conditional_t<TB, typename Plan::StateT, typename Plan::State8>;
  SA sa[MS];
  SBt sb[NS];
#pragma unroll
  for (int i = 0; i < MS; ++i) {
    if constexpr (TA) sa[i] = pl.initT(k, m0 + BM * i, n0, tid);
    else sa[i] = pl.init8(k, m0 + BM * i, n0, tid);
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    if constexpr (TB) sb[j] = pl.initT(k, m0, n0 + BN * j, tid);
    else sb[j] = pl.init8(k, m0, n0 + BN * j, tid);
  }
  // one register set: a second one, keeping two tiles of global loads in flight, was measured: no gain
  // at the C3 conv and C4 GEMM shapes — the loop is not load-latency-bound
  float ra[MS][8], rb[NS][8];
  bf16x8 pa[MS][3], pb[NS][3];
  f32x16 acc[MS][NS];
#pragma unroll
  for (int i = 0; i < MS; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  auto load = [&](int r) {
#pragma unroll
    for (int i = 0; i < MS; ++i) {
      if constexpr (TA) pl.load_at8(sa[i], r, ra[i]);
      else pl.load_a8(sa[i], r, ra[i]);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if constexpr (TB) pl.load_bt8(sb[j], r, rb[j]);
      else pl.load_b8(sb[j], r, rb[j]);
    }
  };
  auto split_all = [&]() {
#pragma unroll
    for (int i = 0; i < MS; ++i) split3_dot2(ra[i], pa[i][0], pa[i][1], pa[i][2]);
#pragma unroll
    for (int j = 0; j < NS; ++j) split3_dot2(rb[j], pb[j][0], pb[j][1], pb[j][2]);
  };
  auto write_all = [&]() {
#pragma unroll
    for (int i = 0; i < MS; ++i)
#pragma unroll
      for (int t = 0; t < 3; ++t)
        *reinterpret_cast<bf16x8*>(&Lt[i][t][TA ? sidx : zimg(srowA, skA >> 3)]) = pa[i][t];
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int t = 0; t < 3; ++t)
        *reinterpret_cast<bf16x8*>(&Lt[MS + j][t][TB ? sidx : zimg(srowB, skB >> 3)]) = pb[j][t];
  };
  auto tread = [&](const __bf16* img, const int (&off)[2], int s) -> bf16x8 {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off[0] + 1024 * s));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off[1] + 1024 * s));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  auto compute_tile = [&]() {
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        bf16x8 fa[MS][3], fb[NS][3];
#pragma unroll
        for (int i = 0; i < MS; ++i)
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            if constexpr (TA) fa[i][q] = tread(Lt[i][q], ra_off, s);
            else fa[i][q] = *reinterpret_cast<const bf16x8*>(&Lt[i][q][zimg(32 * wm + l32, 2 * s + h)]);
          }
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            if constexpr (TB) fb[j][q] = tread(Lt[MS + j][q], rb_off, s);
            else fb[j][q] = *reinterpret_cast<const bf16x8*>(&Lt[MS + j][q][zimg(32 * wn + l32, 2 * s + h)]);
          }
        mfma6_blocks<MS, NS>(acc, fa, fb);
      }
  };
  const int ntile = rend > rbeg ? (rend - rbeg + BK - 1) / BK : 0;
  if (ntile > 0) {
    const int rlast = rbeg + (ntile - 1) * BK;
    load(rbeg);
    split_all();
    write_all();
    load(std::min(rbeg + BK, rlast));
    __syncthreads();
    // one K-tile: the MFMAs of tile t from the LDS images, the split of tile t+1
    // between them, its stash, then the global loads of tile t+2 into the
    // registers just freed (clamped past the last tile: duplicates)
    auto tile_body = [&](int t) {
      const int r0 = rbeg + t * BK;
      compute_tile();
      split_all();
      __syncthreads();  // every wave's fragment reads of tile t are done
      write_all();
      load(std::min(r0 + 2 * BK, rlast));
      __syncthreads();
    };
    for (int t = 0; t < ntile; ++t) tile_body(t);
  }
  const TileOffs<MS, NS> off = sub_tiles<MS, NS>(wm, wn);
  store_tiles<Plan, MS, NS>(pl, S, part, k, split, m0, n0, h, l32, M, N, acc, off);
  if constexpr (has_sq<Plan>::value) {
    if (S == 1 && pl.sq) {
      __shared__ double red[THREADS / 64];
      store_sumsq(pl, k, bx, by, m0, n0, h, l32, M, N, acc, off, red);
    }
  }
}

// ---- the resident weight gradient (layer1) ---------------------------------------
// wsgemm_kernel runs one workgroup per (tap, split-K part): the nine workgroups of a
// part load, split and stash the SAME dy tile, and x tiles that are the same 64
// channels x pixels shifted by the tap's (dh, dw) inside each image.  Here a
// workgroup owns TG taps of one part and walks the part's pixels in chunks of
// RW_PIX = 64 (whole images: H W divides 64; two K-tiles).  Per chunk x (unshifted)
// and dy are loaded, split and stashed once into transposed term images
// [pixel][64 channels] (16-B chunks swizzled by tswz of the STORED pixel row; the x
// images carry a zero row 64), and a tap's x fragment is the two transposed reads
// whose lanes point at k-row pixel + dh W + dw of the same image, or at the zero
// row where load_at8's predicate fails: lane 4q + p of a 16-lane group supplies
// k-row q's address, so the shift is a per-lane choice of row.  Every lane reads
// (EXEC all ones), every address is 8-byte aligned.  The dy fragments of a k-step
// feed all TG taps.
// A split-K part may begin or end in the middle of a chunk (B = 33 at 8 x 8): the
// chunk's images are staged whole and only the part's own K-tiles are multiplied.
// Per accumulator: K-tiles ascending, two k-steps each, wsgemm_kernel's six
// products — bit-identical dw, partials and clip-norm slots (slot = the tap's tile).
// Grid (1, ntaps / TG, K S).  LDS 24,960 B (x) + 24,576 B (dy) = 49,536 B: three
// workgroups per CU, for which the kernel is held to 168 VGPRs.
//
// Banks: a 32-lane half of a transposed read takes four k-rows r .. r + 3; rows of one
// parity share 32 banks, and tswz puts r and r + 2 into different halves of the 128-B
// row only for r % 4 == 0, so a dw = +-1 tap reads 2-way conflicted.  A swizzle that
// holds for every r (bit 1 of the row into bit 2 of the chunk XOR, four zero rows so
// a padded lane keeps its row's low bits: no conflict in the bank model) measured
// the same time: the conflicts are hidden.
constexpr int RW_PIX = 64;                  // pixels per chunk
constexpr int RW_XIMG = (RW_PIX + 1) * 64;  // bf16 per x term image (row 64: zeros)
constexpr int RW_YIMG = RW_PIX * 64;        // bf16 per dy term image
constexpr int RW_TG = 3;                    // taps per workgroup (one kernel row of a 3 x 3)

template <class Plan, int TG>
__global__ __launch_bounds__(THREADS, 3) void rwgemm_kernel(const Plan pl, int S, float* __restrict__ part, int remap) {
  __shared__ __attribute__((aligned(16))) __bf16 Lx[3][RW_XIMG];
  __shared__ __attribute__((aligned(16))) __bf16 Ly[3][RW_YIMG];
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  if (remap >> 8) odd_slot_controls(remap);
  const Geom& g = pl.g;
  const int k = bz / S, split = bz % S;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
  const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
  const int slot0 = by * TG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  const int HW = g.H * g.W;

  // loads: thread (pixel tid & 63 of the chunk, channels 32 c + 8 (tid >> 6) .. +7): a
  // wave reads 64 consecutive pixels of one channel per instruction
  const rsrc_t rx = make_rsrc(pl.x + k * g.sxk, g.xext), ry = make_rsrc(pl.dy + k * g.syk, g.yext);
  const int lp = tid & 63, cg = tid >> 6;
  const int sxc4 = (int)g.sxc * 4, syc4 = (int)g.syc * 4;
  float rxv[2][8], ryv[2][8];
  auto load = [&](int c0) {
    const int q = c0 + lp;
    const uint32_t bb = udiv((uint32_t)q, g.d_hw);
    const int p = q - (int)bb * HW;
    const unsigned vx = q < R ? (unsigned)((int)(bb * g.sxb) + p) * 4u + (unsigned)(8 * cg * sxc4) : SENT;
    const unsigned vy = q < R ? (unsigned)q * 4u + (unsigned)(8 * cg * syc4) : SENT;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        rxv[c][e] = ld1(rx, vx, (32 * c + e) * sxc4);
        ryv[c][e] = ld1(ry, vy, (32 * c + e) * syc4);
      }
  };
  // stash: the thread's 16-B chunks (8 channels of its pixel row) of the six images
  const int sidx = lp * 64 + 8 * (cg ^ tswz(lp));  // channel chunk cg; chunk cg + 4: ^ 32
  bf16x8 px[2][3], py[2][3];
  auto split_all = [&]() {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      split3_dot2(rxv[c], px[c][0], px[c][1], px[c][2]);
      split3_dot2(ryv[c], py[c][0], py[c][1], py[c][2]);
    }
  };
  auto write_all = [&]() {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        *reinterpret_cast<bf16x8*>(&Lx[t][sidx ^ (32 * c)]) = px[c][t];
        *reinterpret_cast<bf16x8*>(&Ly[t][sidx ^ (32 * c)]) = py[c][t];
      }
  };

  // transposed-read lane addresses (bf16 index in a term image).  This lane supplies
  // k-row gq of each 4-row block; its 8-k fragment of k-step (kt, s) is the blocks at
  // chunk pixel 32 kt + 16 s + 8 h + 4 j, j = 0, 1.  dy: the row's swizzle depends on
  // 4 j + gq only, so (kt, s) is a constant offset.  x: per tap, the shifted row or
  // the zero row — two 16-bit indices per register.
  const int gq = (lane & 15) >> 2, gp = lane & 3, g1 = (lane >> 4) & 1;
  const int ca = 4 * wm + 2 * g1 + (gp >> 1), cb = 4 * wn + 2 * g1 + (gp >> 1);
  int yoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kk = 8 * h + 4 * j + gq;
    yoff[j] = kk * 64 + 8 * (cb ^ tswz(kk)) + 4 * (gp & 1);
  }
  unsigned xoff[TG][4];
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    int kh, kw;
    slot_tap(g, slot0 + t, kh, kw);
    const int dh = uni(kh) - g.pad, dw = uni(kw) - g.pad;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      unsigned pk = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int pix = 16 * ks + 8 * h + 4 * j + gq;  // chunk pixel; the chunk starts an image
        const uint32_t bb = udiv((uint32_t)pix, g.d_hw);
        const int p = pix - (int)bb * HW;
        const int oh = (int)udiv((uint32_t)p, g.d_w), ow = p - oh * g.W;
        const int ih = oh + dh, iw = ow + dw;
        const bool ok = (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
        const int sr = ok ? pix + dh * g.W + dw : RW_PIX;
        pk |= (unsigned)(sr * 64 + 8 * (ca ^ tswz(sr)) + 4 * (gp & 1)) << (16 * j);
      }
      xoff[t][ks] = pk;
    }
  }

  f32x16 acc[TG][1][1];
#pragma unroll
  for (int t = 0; t < TG; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][0][0][e] = 0.f;
  auto tread = [&](const __bf16* img, int o0, int o1) -> bf16x8 {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + o1));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  // the chunk's K-tiles that lie in this part, tap by tap inside a k-step
  auto compute_chunk = [&](int c0) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int r0 = c0 + BK * kt;
      if (r0 < rbeg || r0 >= rend) continue;  // workgroup-uniform
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * kt + s;
        bf16x8 fy[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) fy[q] = tread(Ly[q], yoff[0] + 1024 * ks, yoff[1] + 1024 * ks);
#pragma unroll
        for (int t = 0; t < TG; ++t) {
          bf16x8 fx[3];
          const int o0 = (int)(xoff[t][ks] & 0xffffu), o1 = (int)(xoff[t][ks] >> 16);
#pragma unroll
          for (int q = 0; q < 3; ++q) fx[q] = tread(Lx[q], o0, o1);
          acc[t][0][0] = mfma6(acc[t][0][0], fx, fy);
        }
      }
    }
  };
  if (rend > rbeg) {
    const int cbeg = rbeg / RW_PIX * RW_PIX;
    const int nchunk = (rend - cbeg + RW_PIX - 1) / RW_PIX;
    const int clast = cbeg + (nchunk - 1) * RW_PIX;
    load(cbeg);
    if (tid < 24) {  // the zero row of the three x images: eight 16-B chunks each
      bf16x8 z;
#pragma unroll
      for (int q = 0; q < 8; ++q) z[q] = (__bf16)0.f;
      *reinterpret_cast<bf16x8*>(&Lx[0][0] + (tid >> 3) * RW_XIMG + RW_PIX * 64 + 8 * (tid & 7)) = z;
    }
    split_all();
    write_all();
    load(std::min(cbeg + RW_PIX, clast));
    __syncthreads();
    // one chunk: its MFMAs from the images and the split of the next chunk; then, once
    // every wave's fragment reads are done, that chunk's stash and the global loads of
    // the one after (clamped past the last chunk: duplicates).  Splitting after the
    // barrier instead measured 116.4–117.7 against 114.9–115.4 us at l1.
    for (int c = 0; c < nchunk; ++c) {
      const int c0 = cbeg + c * RW_PIX;
      compute_chunk(c0);
      split_all();
      __syncthreads();
      write_all();
      load(std::min(c0 + 2 * RW_PIX, clast));
      __syncthreads();
    }
  }
  const TileOffs<1, 1> off = sub_tiles<1, 1>(wm, wn);
#pragma unroll
  for (int t = 0; t < TG; ++t)
    store_tiles<Plan, 1, 1>(pl, S, part, k, split, (slot0 + t) * BM, 0, h, l32, M, N, acc[t], off);
  if constexpr (has_sq<Plan>::value) {
    if (S == 1 && pl.sq) {  // one slot per (tap, ci) tile: wsgemm_kernel's by * gridDim.x + bx with gridDim.x = 1
      __shared__ double red[TG][THREADS / 64];
#pragma unroll
      for (int t = 0; t < TG; ++t)
        store_sumsq(pl, k, 0, slot0 + t, (slot0 + t) * BM, 0, h, l32, M, N, acc[t], off, red[t]);
    }
  }
}

template <class Plan>
__global__ void treduce_kernel(const Plan pl, int S, const float* __restrict__ part) {
  // grid (cdiv(M*N, 256), K): one client per grid row, 32-bit index math
  const int M = pl.M(), N = pl.N(), K = pl.g.Kc;
  const int k = blockIdx.y;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t MN = (int64_t)M * N;
  float v = 0.f;
  if (e < MN) {
    const int m = e / N, n = e - m * N;
    const int64_t idx = k * MN + e;
    v = part[idx];
    for (int s = 1; s < S; ++s) v += part[(int64_t)s * MN * K + idx];
    pl.store(k, m, n, v);
  }
  if constexpr (has_sq<Plan>::value) {
    if (pl.sq) {  // this block's clip-norm partial (slot = blockIdx.x)
      __shared__ double red[4];
      const double t = block_sumsq((double)v * (double)v, red);
      if (threadIdx.x == 0) pl.sq[(int64_t)k * pl.sq_ld + blockIdx.x] = t;
    }
  }
}

}  // namespace convt
}  // namespace flr

#ifdef FLR_ABLATION
#include "conv_t_ablation.h"  // the tools build's kernel forms: they use the epilogue above
#endif
