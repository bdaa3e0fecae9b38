// The fused strided data gradient (stride 2, H and W even): ONE launch per conv
// instead of one per stride-parity class plus their split-K reduce passes.
//
// A workgroup owns an M-tile of input channels and one column tile of the
// classes' common GEMM (all four classes have the same Hc x Wc, so column n is
// the same (image, ihc, iwc) in each: the workgroup owns every parity class of
// its pixels).  For each class in turn — (0,0), (0,1), (1,0), (1,1),
// dgrad_classes' order — it runs sgemm_body's K-loop with that class's DgradT
// plan: the same init8 / load_a8 / load_b8, K-tile order, k-steps and six
// products per accumulator.  Where the per-class launch takes split-K S > 1
// (resolve()'s S for that class and workspace), the S ranges of K-tiles run one
// after another into a fresh accumulator each and are summed in
// treduce_kernel's order (part 0, + part 1, ...): the same bits, no partial
// written, no reduce launch.  The optional shortcut (the block's 1x1 / 2
// projection, today a second call accumulating in place onto class (0, 0)) is
// one more K-loop on its own dy and weights; dx = fadd(shortcut, conv result),
// the in-place call's operand order.
//
// Stores: a lane's column holds horizontally adjacent pixels in classes (ca, 0)
// and (ca, 1), so the finished (ca, 0) values wait in an LDS slab of the
// thread's own slots (no barrier) and leave with (ca, 1)'s as one 8-byte store;
// the lanes of a class row then write a whole contiguous row of dx.
#pragma once

#include "conv_t_launch.h"

namespace flr {
namespace convt {

constexpr int FD_CLASSES = 4;  // stride 2, H and W even

struct DgradFusedArgs {
  DgradT cls[FD_CLASSES];
  DgradT sc;           // the shortcut's class (0, 0) (Ssc > 0)
  int S[FD_CLASSES];   // the per-class launch's split-K count
  int Ssc;             // the shortcut launch's; 0: no shortcut
};

// sgemm_body's K-loop over the S split ranges of pl's reduction, summed in
// treduce_kernel's order into run.  Ends on a barrier: Ls is free afterwards.
template <int MS, int NS, bool NAR, int MSW>
__device__ __forceinline__ void fd_ksum(const DgradT& pl, int S, int k, int m0, int n0,
                                        __bf16 (&Ls)[MS + NS][3][TERM_B], f32x16 (&run)[MSW][NS]) {
  const int R = pl.R();
  const int ktiles = cdiv(R, BK);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  const int srowA = stash_row<DgradT::QUAD_A>(tid), skA = stash_k<DgradT::QUAD_A>(tid);
  const int srowB = stash_row<DgradT::QUAD_B>(tid), skB = stash_k<DgradT::QUAD_B>(tid);
  typename DgradT::State8 sa[MS], sb[NS];
#pragma unroll
  for (int i = 0; i < MS; ++i) sa[i] = pl.init8(k, m0 + BM * i, n0, tid);
#pragma unroll
  for (int j = 0; j < NS; ++j) sb[j] = pl.init8(k, m0, n0 + BN * j, tid);
  float ra[MS][8], rb[NS][8];
  bf16x8 pa[MS][3], pb[NS][3];
  f32x16 acc[MSW][NS];
  auto a_sub = [&](int i) { return NAR ? (wave * MSW + i) >> 1 : i; };
  auto a_row = [&](int i) { return NAR ? 32 * ((wave * MSW + i) & 1) + l32 : 32 * wm + l32; };
  auto b_row = [&]() { return NAR ? l32 : 32 * wn + l32; };
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
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < NKS; ++s) mfma6_blocks<MSW, NS>(acc, fa[s], fb[s]);
  };
  for (int split = 0; split < S; ++split) {
    const int rbeg = (int)((int64_t)ktiles * split / S) * BK;
    const int rend = std::min(R, (int)((int64_t)ktiles * (split + 1) / S) * BK);
#pragma unroll
    for (int i = 0; i < MSW; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int ntile = rend > rbeg ? (rend - rbeg + BK - 1) / BK : 0;
    if (ntile > 0) {
      const int rlast = rbeg + (ntile - 1) * BK;
      load(rbeg);
      split_all();
      write_all();
      load(std::min(rbeg + BK, rlast));
      __syncthreads();
      for (int t = 0; t < ntile; ++t) {
        const int r0 = rbeg + t * BK;
        compute_tile();
        split_all();
        __syncthreads();
        write_all();
        load(std::min(r0 + 2 * BK, rlast));
        __syncthreads();
      }
    }
#pragma unroll
    for (int i = 0; i < MSW; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) run[i][j][e] = split == 0 ? acc[i][j][e] : __fadd_rn(run[i][j][e], acc[i][j][e]);
  }
}

template <int MS, int NS, bool NAR>
__global__ __launch_bounds__(THREADS, SG_OCC) void fdgrad_kernel(const DgradFusedArgs fa, int remap, int rows) {
  constexpr int MSW = NAR ? MS / 2 : MS;
  __shared__ __attribute__((aligned(16))) __bf16 Ls[MS + NS][3][TERM_B];
  __shared__ float Lh[MSW * NS * 16][THREADS];  // slot [block element][thread]: conflict-free, thread-private
  int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (remap & 1) xcd_tile(bx, by, bz);
  const int k = bz;
  // rows: the two class rows (ca = 0: classes (0, 0), (0, 1) and the shortcut; ca = 1)
  // of a tile in two workgroups, neighbours in x — half the serial K-tiles each
  const int c0 = rows ? 2 * (bx & 1) : 0, c1 = rows ? c0 + 2 : FD_CLASSES;
  if (rows) bx >>= 1;
  const DgradT& p0 = fa.cls[0];
  const Geom& g = p0.g;
  const int M = p0.M(), N = p0.N();  // every class: the same M and N
  const int m0 = by * BM * MS, n0 = bx * BN * NS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l32 = lane & 31;
  // this wave's block (i, j): row / column offset from (m0, n0) (sgemm_body's m_off / n_off)
  auto m_off = [&](int i) { return NAR ? 32 * (wave * MSW + i) : BM * i + 32 * wm; };
  auto n_off = [&](int j) { return NAR ? 0 : BN * j + 32 * wn; };
  // column n -> float offset of its class-(0, 0) pixel in dx, less the channel term (-1: past N)
  int col[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int n = n0 + n_off(j) + l32;
    const DgradT::Col c = p0.col(n);
    col[j] = n < N ? (int)(k * g.sxk + c.bb * g.sxb + 2 * c.ihc * g.W + 2 * c.iwc) : -1;
  }
  f32x16 run[MSW][NS];
  if (fa.Ssc > 0 && c0 == 0) {  // the shortcut's gradient first: it waits in the slab for class (0, 0)
    fd_ksum<MS, NS, NAR, MSW>(fa.sc, fa.Ssc, k, m0, n0, Ls, run);
#pragma unroll
    for (int i = 0; i < MSW; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) Lh[(i * NS + j) * 16 + e][tid] = run[i][j][e];
  }
  for (int c = c0; c < c1; ++c) {
    const DgradT& pl = fa.cls[c];
    const int ca = c >> 1, cb = c & 1;
    fd_ksum<MS, NS, NAR, MSW>(pl, fa.S[c], k, m0, n0, Ls, run);
    const float* add = pl.add;
    const int coff = ca * g.W + cb;
#pragma unroll
    for (int i = 0; i < MSW; ++i)
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        int ix[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + m_off(i) + (e & 3) + 8 * (e >> 2) + 4 * h;
          ix[e] = (m < M && col[j] >= 0) ? col[j] + m * (int)g.sxc + coff : -1;
        }
        if (add) {  // the addends loaded before any store (add may be dx)
          float av[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) av[e] = ix[e] >= 0 ? add[ix[e]] : 0.f;
#pragma unroll
          for (int e = 0; e < 16; ++e) run[i][j][e] = __fadd_rn(run[i][j][e], av[e]);
        }
        if (c == 0 && fa.Ssc > 0) {  // the in-place shortcut call's add: dgrad(shortcut) + dx
#pragma unroll
          for (int e = 0; e < 16; ++e) run[i][j][e] = __fadd_rn(Lh[(i * NS + j) * 16 + e][tid], run[i][j][e]);
        }
        if (cb == 0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) Lh[(i * NS + j) * 16 + e][tid] = run[i][j][e];
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (ix[e] >= 0)
              *reinterpret_cast<float2*>(pl.dx + (ix[e] - 1)) = make_float2(Lh[(i * NS + j) * 16 + e][tid], run[i][j][e]);
        }
      }
  }
}

// FLR_DGRAD_FUSED (read per launch): 0 = the per-class launches, 1 = the fused
// kernel wherever eligible, unset = the per-shape preference below.
inline int dgrad_fused_knob() {
  const char* e = flr::knob("FLR_DGRAD_FUSED");
  if (!e || !e[0]) return -1;
  return e[0] == '0' ? 0 : 1;
}

// The geometry the fused kernel covers: stride 2 with H and W even (four classes
// of equal size), the split-at-stash form.
inline bool dgrad_fused_geom_ok(const Geom& g) {
  return g.stride == 2 && g.H % 2 == 0 && g.W % 2 == 0 && gemm_form() == 5;
}

// Column tile of the classes' GEMM (M = Cin rows, N = B * Hc * Wc columns per
// class): the narrow tile (code 20) where a class has at most 32 columns (l4a),
// 64 x 128 (12) for 64 input channels (l2a), else 64 x 64 (11) — and the grid.
inline int fd_tile(int M, int N) {
  if (narrow_shape(M, N)) return 20;
  return M == BM && N % (2 * BN) == 0 ? 12 : 11;
}
// The two class rows of a tile in two workgroups (fdgrad_kernel's rows): taken for the
// narrow tile when the second row has taps — its grid is otherwise one workgroup per
// CU at 128 clients with 80 K-tiles in a row (l4a + shortcut 132 -> 99 us, l4a alone
// 107 -> 70; the wider tiles, already two workgroups per CU, lose 5-15 % to it).
// FLR_DGRAD_FUSED_ROWS=0|1 forces it off / on (A/B, read per launch).
inline int fd_rows(int tile, bool row1_taps) {
  const char* e = flr::knob("FLR_DGRAD_FUSED_ROWS");
  if (e && e[0]) return e[0] == '0' ? 0 : 1;
  return tile == 20 && row1_taps ? 1 : 0;
}
inline dim3 fd_grid(int M, int N, int K, int rows) {
  const unsigned r = rows ? 2u : 1u;
  switch (fd_tile(M, N)) {
    case 20: return dim3(r, (unsigned)(M / (2 * BM)), (unsigned)K);
    case 12: return dim3(r * (unsigned)(N / (2 * BN)), 1u, (unsigned)K);
    default: return dim3(r * (unsigned)cdiv(N, BN), (unsigned)cdiv(M, BM), (unsigned)K);
  }
}

// Where alternated tools/conv_bench.py runs showed the fused form faster than the
// per-class launches on MI355X (profiles/dgrad_fused/README.md; K = 128, B = 32):
// l2a, l3a, l4a and the three 1x1 shortcuts, alone or with the shortcut folded in.
// A fused workgroup runs its classes' K-tiles one after another, so the form needs
// its own grid to fill the chip: only grids of at least one column tile per CU were
// measured, smaller ones (few clients per GPU) keep the per-class launches and
// their split-K.
constexpr int FD_MIN_WG = 256;
inline bool dgrad_fused_preferred(const Geom& g, bool shortcut) {
  (void)shortcut;
  const int M = g.Cin, N = g.B * (g.H / 2) * (g.W / 2);
  const dim3 grid = fd_grid(M, N, g.Kc, 0);  // tiles, whether or not their class rows are split
  return (int64_t)grid.x * grid.y * grid.z >= FD_MIN_WG;
}

// Which form a call runs: the geometry, the knob / preference, and the operands
// (8-byte stores need dx 8-byte aligned; an in-place call that skips its empty
// classes keeps the per-class path).
inline bool dgrad_fused_ok(const Geom& g, const DgradT* cls, int nc, const float* add, const float* dx,
                           const Geom* gsc) {
  if (!dgrad_fused_geom_ok(g) || nc != FD_CLASSES) return false;
  const int kn = dgrad_fused_knob();
  if (kn == 0 || (kn < 0 && !dgrad_fused_preferred(g, gsc != nullptr))) return false;
  if (reinterpret_cast<uintptr_t>(dx) & 7) return false;
  for (int c = 0; c < nc; ++c)
    if (add == dx && cls[c].R() == 0) return false;
  if (gsc && !(gsc->stride == 2 && gsc->Kc == g.Kc && gsc->B == g.B && gsc->Cin == g.Cin && gsc->H == g.H &&
               gsc->W == g.W))
    return false;
  return true;
}

inline int launch_dgrad_fused(const DgradFusedArgs& fa, hipStream_t st, const char* name) {
  const DgradT& p0 = fa.cls[0];
  const int M = p0.M(), N = p0.N(), K = p0.g.Kc;
  const int tile = fd_tile(M, N), rows = fd_rows(tile, fa.cls[2].R() + fa.cls[3].R() > 0);
  const dim3 grid = fd_grid(M, N, K, rows);
  switch (tile) {
    case 20:
      hipLaunchKernelGGL((fdgrad_kernel<2, 1, true>), grid, dim3(THREADS), 0, st, fa, xcd_remap() & 1, rows);
      break;
    case 12:
      hipLaunchKernelGGL((fdgrad_kernel<1, 2, false>), grid, dim3(THREADS), 0, st, fa, xcd_remap() & 1, rows);
      break;
    default:
      hipLaunchKernelGGL((fdgrad_kernel<1, 1, false>), grid, dim3(THREADS), 0, st, fa, xcd_remap() & 1, rows);
  }
  return launch_status(name);
}

}  // namespace convt
}  // namespace flr
