// The batched-GEMM kernel forms that were measured slower than split-at-stash
// and the knobs that select them: the LDS-DMA form (dsgemm_kernel), the
// pre-split form (presplit_kernel + psgemm_kernel) and transposed images for
// k-contiguous operands; with them the timing ablations of the split-at-stash
// loop (FLR_SG_ABL) and the tgemm forms 1, 3 and 4.  Compiled into the tools
// build only (make ABLATION=1): conv_t_kernels.h includes this file after its
// kernels, and launch_tiles (conv_t_launch.h) asks launch_ablation() first.
#pragma once

#include <climits>

namespace flr {
namespace convt {

// ---- the LDS-DMA form (FLR_BGEMM_DMA=1, batched GEMMs with RK / KR operands) ---
// 128 x 128 tiles, four waves of 64 x 64.  The fp32 operand tiles go global ->
// LDS by buffer_load_dwordx4 ... lds (BGemm::dma_op): no VGPR staging and no
// ds_write pass (the split-at-stash form spends 36 % of its loop in the stash
// writes, profiles/r3_gemm_loop/).  Two LDS stages of 32 KB, one barrier per
// K-tile: tile t+1's DMA runs under tile t's MFMAs.  Each wave splits its own
// fragments into bf16 hi / mid / lo at read time (twice the split work of the
// stash form, on the VALU beside the MFMAs).  Every accumulator sees the same
// bf16 products in the same order as sgemm_body: bit-identical.
constexpr int DG_IMG = 128 * BK;  // floats per operand image
template <class Plan>
__global__ __launch_bounds__(THREADS, 2) void dsgemm_kernel(const Plan pl, int S, float* __restrict__ part,
                                                            int remap) {
  constexpr int MSW = 2, NS = 2;
  __shared__ __attribute__((aligned(16))) float Lf[2][2][DG_IMG];  // [stage][A, B]
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  const int k = bz / S, split = bz % S;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
  const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
  const int m0 = by * 128, n0 = bx * 128;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  const typename Plan::State8 st = pl.init8(k, m0, n0, tid);
  f32x16 acc[MSW][NS];
#pragma unroll
  for (int i = 0; i < MSW; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  auto dma = [&](int r0, int sg) {
    pl.dma_a(st, &Lf[sg][0][0], r0, wave, lane);
    pl.dma_b(st, &Lf[sg][1][0], r0, wave, lane);
  };
  // lane (l32, h): row `row` of the image, k = 16 s + 8 h .. +7
  auto frag = [&](const float* img, auto modec, int row, int s, float (&v)[8]) {
    constexpr int MODE = decltype(modec)::value;
    if constexpr (MODE == BM_RK) {
      const int f = (row >> 1) & 7, q0 = 4 * s + 2 * h;
      const f32x4 a = *reinterpret_cast<const f32x4*>(img + row * BK + 4 * (q0 ^ f));
      const f32x4 b = *reinterpret_cast<const f32x4*>(img + row * BK + 4 * ((q0 + 1) ^ f));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = a[e];
        v[4 + e] = b[e];
      }
    } else {
      const float* p = img + (16 * s + 8 * h) * 128 + 4 * ((row >> 2) ^ (h << 3)) + (row & 3);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = p[e * 128];
    }
  };
  using MA = std::integral_constant<int, Plan::AMODE>;
  using MB = std::integral_constant<int, Plan::BMODE>;
  auto compute = [&](int sg) {
    const float* ia = &Lf[sg][0][0];
    const float* ib = &Lf[sg][1][0];
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 fa[MSW][3], fb[NS][3];
#pragma unroll
      for (int i = 0; i < MSW; ++i) {
        float v[8];
        frag(ia, MA{}, 64 * i + 32 * wm + l32, s, v);
        split3_dot2(v, fa[i][0], fa[i][1], fa[i][2]);
      }
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        float v[8];
        frag(ib, MB{}, 64 * j + 32 * wn + l32, s, v);
        split3_dot2(v, fb[j][0], fb[j][1], fb[j][2]);
      }
      mfma6_blocks<MSW, NS>(acc, fa, fb);
    }
  };
  const int ntile = rend > rbeg ? (rend - rbeg + BK - 1) / BK : 0;
  if (ntile > 0) {
    dma(rbeg, 0);
    for (int t = 0; t < ntile; ++t) {
      // this wave's DMA of tile t landed; after the barrier every wave's has, and
      // every wave's fragment reads of tile t-1 (the stage refilled next) are done
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
      if (t + 1 < ntile) dma(rbeg + (t + 1) * BK, (t + 1) & 1);
      compute(t & 1);
    }
  }
  store_tiles<Plan, MSW, NS>(pl, S, part, k, split, m0, n0, h, l32, M, N, acc, sub_tiles<MSW, NS>(wm, wn));
}

// FLR_BGEMM_DMA=1 selects the LDS-DMA form (read per launch).  Off by default:
// bit-identical, but 0-18 % SLOWER than split-at-stash at every C4 encoder shape
// (vit.qkv 461 vs 391 us, vit.fc1 519 vs 489, vit.fc2 480 vs 455 at 32 clients;
// profiles/r4_bgemm_dma_ab.txt): the per-wave split doubles the VALU split work
// of the stash form, which costs more than the ds_write pass it removes.
inline bool bgemm_dma() { return knob_on("FLR_BGEMM_DMA"); }
// ---- the pre-split form (batched GEMMs with 128 x 128 tiles, FLR_BGEMM_PRESPLIT=1; measured slower) --
// Each operand is split into bf16 hi / mid / lo ONCE per GEMM by presplit_kernel
// (the same split3_dot2 as every other form) into k-contiguous planes in the
// workspace, [3][K][rows_pad][R_pad] with rows padded to 128 and R to 32 by
// zeros.  The GEMM (psgemm_kernel) is then a plain six-product bf16 loop: each
// 16-deep k-step's three A and three B planes go global -> LDS by
// buffer_load_dwordx4 ... lds into a ring of three 24-KB stages (two k-steps in
// flight, counted vmcnt, raw barrier), fragments are one ds_read_b128 per term,
// no VGPR staging, no ds_write, no split in the loop.  Same bf16 terms, same
// products in the same order per accumulator: bit-identical to sgemm_body.
constexpr int PS_ROWS = 128;                 // tile rows per operand
constexpr int PS_PLANE = PS_ROWS * 16;       // bf16 per plane per stage (16 k per row)
constexpr int PS_STAGE = 6 * PS_PLANE;       // A hi/mid/lo, B hi/mid/lo
constexpr int PS_NST = 3;                    // ring stages
constexpr int PS_PIECES = 6 * PS_PLANE * 2 / 1024;  // 1-KB DMA pieces per stage (24)
static_assert(PS_PIECES % 4 == 0, "pieces split over four waves");

inline int64_t ps_pad(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline size_t ps_plane_bytes(int64_t K, int64_t rows, int64_t R) {
  return (size_t)3 * K * ps_pad(rows, PS_ROWS) * ps_pad(R, BK) * 2;
}

// planes[t][k][row][c] = term t of src(k, row, c) (0 outside rows x R)
template <int MODE>
__global__ __launch_bounds__(THREADS) void presplit_kernel(const float* __restrict__ src, int64_t s_k, int64_t s_row,
                                                           int64_t s_r, int K, int rows, int R, int rows_pad,
                                                           int R_pad, __bf16* __restrict__ planes) {
  const int ngrp = R_pad / 8;  // 8-wide k groups per row
  const int64_t per_k = (int64_t)rows_pad * ngrp;
  const int64_t total = (int64_t)K * per_k;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
    const int k = (int)(i / per_k);
    const int64_t rem = i - (int64_t)k * per_k;
    int row, grp;
    if constexpr (MODE == BM_RK) {  // lanes along k: each reads 32 contiguous bytes
      row = (int)(rem / ngrp);
      grp = (int)(rem - (int64_t)row * ngrp);
    } else {  // lanes along rows: each load instruction reads consecutive rows
      grp = (int)(rem / rows_pad);
      row = (int)(rem - (int64_t)grp * rows_pad);
    }
    float v[8];
    const float* base = src + k * s_k + (int64_t)row * s_row;
    if constexpr (MODE == BM_RK) {  // s_r == 1, R % 4 == 0, 16-B aligned rows: two float4 loads
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = 8 * grp + 4 * q;
        const f32x4 x = (row < rows && c < R) ? *reinterpret_cast<const f32x4*>(base + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = x[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 8 * grp + e;
        v[e] = (row < rows && c < R) ? base[(int64_t)c * s_r] : 0.f;
      }
    }
    bf16x8 t0, t1, t2;
    split3_dot2(v, t0, t1, t2);
    const int64_t plane = (int64_t)K * rows_pad * R_pad;
    const int64_t o = ((int64_t)k * rows_pad + row) * R_pad + 8 * grp;
    *reinterpret_cast<bf16x8*>(planes + o) = t0;
    *reinterpret_cast<bf16x8*>(planes + plane + o) = t1;
    *reinterpret_cast<bf16x8*>(planes + 2 * plane + o) = t2;
  }
}

template <class Plan>
__global__ __launch_bounds__(THREADS, 2) void psgemm_kernel(const Plan pl, int S, float* __restrict__ part, int remap,
                                                            const __bf16* __restrict__ pa, const __bf16* __restrict__ pb,
                                                            int Mp, int Np, int Rp) {
  constexpr int MSW = 2, NS = 2;
  __shared__ __attribute__((aligned(16))) __bf16 L[PS_NST * PS_STAGE];  // one array: no compiler vmcnt(0)
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  const int k = bz / S, split = bz % S;
  const int M = pl.M(), N = pl.N(), R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
  const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
  const int m0 = by * 128, n0 = bx * 128;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  // plane (operand o, term t) of client k: rows from m0 / n0, all of R_pad
  const int64_t pla = (int64_t)pl.g.Kc * Mp * Rp, plb = (int64_t)pl.g.Kc * Np * Rp;
  const rsrc_t ra = make_rsrc(reinterpret_cast<const float*>(pa), 3 * pla / 2);
  const rsrc_t rb = make_rsrc(reinterpret_cast<const float*>(pb), 3 * plb / 2);
  f32x16 acc[MSW][NS];
#pragma unroll
  for (int i = 0; i < MSW; ++i)
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // one 16-deep k-step into ring stage sg: piece p = (operand, term, 32-row block);
  // lane: row (lane >> 1) of the block, its 16-B half (lane & 1) holds the k half
  // (lane & 1) ^ ((row >> 3) & 1) (source-side swizzle)
  auto dma = [&](int k0, int sg) {
#pragma unroll
    for (int q = 0; q < PS_PIECES / 4; ++q) {
      const int piece = (PS_PIECES / 4) * wave + q;
      const int op = piece / 12, t = (piece % 12) / 4, blk = piece % 4;
      const int row = 32 * blk + (lane >> 1);
      const int half = (lane & 1) ^ ((row >> 3) & 1);
      const int64_t rows_pad = op ? Np : Mp;
      const int64_t e = (int64_t)t * (op ? plb : pla) + ((int64_t)k * rows_pad + (op ? n0 : m0) + row) * Rp + k0 +
                        8 * half;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(op ? rb : ra,
                                               (__attribute__((address_space(3))) void*)(L + sg * PS_STAGE +
                                                                                        piece * 512),
                                               16, (unsigned)(e * 2), 0, 0, 0);
    }
  };
  auto frag = [&](int sg, int op, int t, int row) {
    const int off = sg * PS_STAGE + (op * 3 + t) * PS_PLANE + row * 16 + 8 * (h ^ ((row >> 3) & 1));
    return *reinterpret_cast<const bf16x8*>(L + off);
  };
  const int nstep = rend > rbeg ? 2 * ((rend - rbeg + BK - 1) / BK) : 0;
  if (nstep > 0) {
    dma(rbeg, 0);
    if (nstep > 1) dma(rbeg + 16, 1);
    for (int s = 0; s < nstep; ++s) {
      // this wave's DMA of step s landed (step s+1's may still fly); after the
      // barrier every wave's has, and every wave's reads of step s-1 are done
      if (s + 1 < nstep) {
        static_assert(PS_PIECES / 4 == 6, "vmcnt immediate below");
        asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (s + 2 < nstep) dma(rbeg + 16 * (s + 2), (s + 2) % PS_NST);
      const int sg = s % PS_NST;
      bf16x8 fa[MSW][3], fb[NS][3];
#pragma unroll
      for (int i = 0; i < MSW; ++i)
#pragma unroll
        for (int t = 0; t < 3; ++t) fa[i][t] = frag(sg, 0, t, 64 * i + 32 * wm + l32);
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int t = 0; t < 3; ++t) fb[j][t] = frag(sg, 1, t, 64 * j + 32 * wn + l32);
      mfma6_blocks<MSW, NS>(acc, fa, fb);
    }
  }
  store_tiles<Plan, MSW, NS>(pl, S, part, k, split, m0, n0, h, l32, M, N, acc, sub_tiles<MSW, NS>(wm, wn));
}

// FLR_BGEMM_PRESPLIT=1 selects the pre-split form (read per launch and per
// workspace query).  Off by default: bit-identical, but 1.6-3x SLOWER than
// split-at-stash at the C4 encoder shapes (vit.qkv 624 vs 392 us, vit.fc1.dw 1484
// vs 499 us at 32 clients; profiles/r4_bgemm_presplit_ab.txt).  Three bf16 planes
// are 6 B per operand value against the stash form's 4 B of fp32: the 128 x 128
// tiles re-read their operands from L2 once per opposite tile, so the loop moves
// 1.5x the bytes (2.8 GB per vit.qkv GEMM at 32 clients), and the split pass
// itself transposes the row-contiguous (KR) operands of the weight gradients.
inline bool bgemm_presplit() { return knob_on("FLR_BGEMM_PRESPLIT"); }

template <class P> struct dma_ok : std::false_type {};
template <int A, int B> struct dma_ok<BGemm<A, B>> : std::integral_constant<bool, A != BM_G && B != BM_G> {};

// ---- transposed images for the batched GEMM (wsgemm_kernel) --------------------
template <class P> struct is_bgemm_t : std::false_type {
  static constexpr bool ta = false, tb = false;
};
template <int A, int B> struct is_bgemm_t<BGemm<A, B>> : std::true_type {
  static constexpr bool ta = A == BM_RK, tb = B == BM_RK;
};
// FLR_BGEMM_TIMG=1: k-contiguous batched-GEMM operands on transposed images
// (A/B; off by default: the eight 4-B loads per thread cost more than the
// quad-lane stash's 2-way bank conflicts save — vit.qkv 493 vs 426 us at K=32,
// profiles/r3_bgemm_timg.txt)
inline bool bgemm_timg() { return knob_on("FLR_BGEMM_TIMG"); }

// launch_tiles' hook: runs the tools build's form the knobs select for this
// launch, if any (true: launched).  form is gemm_form(); partp moves past the
// planes when the pre-split form takes the front of the workspace.
template <class Plan, int MS, int NS>
bool launch_ablation(const Plan& pl, dim3 grid, int S, int form, void* ws, size_t ws_bytes, hipStream_t st,
                     float*& partp) {
  const int M = pl.M(), N = pl.N(), R = pl.R(), K = pl.g.Kc;
  float* part = static_cast<float*>(ws);
  if constexpr (is_bgemm_t<Plan>::ta || is_bgemm_t<Plan>::tb) {
    // batched GEMMs with a k-contiguous operand: that operand on a transposed
    // image (coalesced 128-B row reads, conflict-free stashes; the row-major
    // image of a quad-lane load stashes 2-way bank-conflicted)
    if (form == 5 && bgemm_timg()) {
      hipLaunchKernelGGL((wsgemm_kernel<Plan, MS, NS, is_bgemm_t<Plan>::ta, is_bgemm_t<Plan>::tb>), grid,
                         dim3(THREADS), 0, st, pl, S, part, xcd_remap());
      return true;
    }
  }
  if constexpr (std::is_base_of<BGemmArgs, Plan>::value && MS == 2 && NS == 2) {
    if (form == 5 && bgemm_presplit()) {
      const size_t pa_b = (ps_plane_bytes(K, M, R) + 255) / 256 * 256;
      const size_t pb_b = (ps_plane_bytes(K, N, R) + 255) / 256 * 256;
      const size_t need = pa_b + pb_b + (S > 1 ? (size_t)S * K * M * N * sizeof(float) : 0);
      // the planes' byte offsets must fit the 31-bit buffer voffset
      if (ws && ws_bytes >= need && pa_b < (size_t(1) << 31) && pb_b < (size_t(1) << 31)) {
        __bf16* pa = static_cast<__bf16*>(ws);
        __bf16* pb = reinterpret_cast<__bf16*>(static_cast<char*>(ws) + pa_b);
        partp = reinterpret_cast<float*>(static_cast<char*>(ws) + pa_b + pb_b);
        const int Mp = (int)ps_pad(M, PS_ROWS), Np = (int)ps_pad(N, PS_ROWS), Rp = (int)ps_pad(R, BK);
        auto pgrid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 16384))); };
        hipLaunchKernelGGL((presplit_kernel<Plan::AMODE>), pgrid((int64_t)K * Mp * Rp / 8), dim3(THREADS), 0, st, pl.a,
                           pl.a_k, pl.a_m, pl.a_r, K, M, R, Mp, Rp, pa);
        hipLaunchKernelGGL((presplit_kernel<Plan::BMODE>), pgrid((int64_t)K * Np * Rp / 8), dim3(THREADS), 0, st, pl.b,
                           pl.b_k, pl.b_n, pl.b_r, K, N, R, Np, Rp, pb);
        hipLaunchKernelGGL((psgemm_kernel<Plan>), grid, dim3(THREADS), 0, st, pl, S, partp, xcd_remap(), pa, pb, Mp,
                           Np, Rp);
        return true;
      }
    }
  }
  if constexpr (dma_ok<Plan>::value && MS == 2 && NS == 2) {
    if (form == 5 && bgemm_dma()) {
      hipLaunchKernelGGL((dsgemm_kernel<Plan>), grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap());
      return true;
    }
  }
  if constexpr (has_k8<Plan>::value && MS == 2 && NS == 2) {
    const int abl = knob_int("FLR_SG_ABL", INT_MIN, INT_MAX, 0);  // timing ablations of the main loop
#define FLR_SG_ABL_CASE(A)                                                                                      \
  if (form == 5 && abl == A) {                                                                                   \
    hipLaunchKernelGGL((sgemm_kernel<Plan, MS, NS, A>), grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap()); \
    return true;                                                                                                 \
  }
    FLR_SG_ABL_CASE(1) FLR_SG_ABL_CASE(2) FLR_SG_ABL_CASE(3) FLR_SG_ABL_CASE(4) FLR_SG_ABL_CASE(8)
    FLR_SG_ABL_CASE(10) FLR_SG_ABL_CASE(16) FLR_SG_ABL_CASE(11) FLR_SG_ABL_CASE(15) FLR_SG_ABL_CASE(23)
#undef FLR_SG_ABL_CASE
  }
  // 1: accumulator-chain order; 3: one bf16 term, no split (wrong results); 4: the unpipelined loop
#define FLR_TG_FORM(F)                                                                                            \
  if (form == F) {                                                                                                 \
    hipLaunchKernelGGL((tgemm_kernel<Plan, MS, NS, F>), grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap(),    \
                       mfma_prio());                                                                               \
    return true;                                                                                                   \
  }
  FLR_TG_FORM(1) FLR_TG_FORM(3) FLR_TG_FORM(4)
#undef FLR_TG_FORM
  return false;
}

}  // namespace convt
}  // namespace flr
