// Reference-exact Krum distances (agg_pairwise_ref.hip), the layout kernels:
// a segment of the client matrix rewritten chain-major (chain_transpose_kernel,
// tap_chain_kernel for the tap-major blocks, zero_slots_kernel for the padding),
// a dead region's dead stream (dead_stream_kernel), and the throughput forms'
// block-major segment (quad_transpose_kernel); their launchers at the end.
#include "pwref_launch.h"

namespace flr {
namespace pwref {

constexpr int TROW = TW + 4;  // LDS floats per chain row
// Xc[k][c][s] = X[k][8 (r0 + s) + c] for s < steps; stream stride ldc (x 8 per row).
// Each wave moves 256 steps (8 KB) on its own: 8 lane-contiguous 16-B loads
// (1 KB per instruction), the floats scattered into a chain-major LDS image
// (rows of 256 + 4 floats: the b32 writes of a 32-lane group hit 32 banks),
// then per chain one 16-B read of 4 steps per lane and a lane-contiguous 1-KB
// store.  (Per-lane 128-B rows read at 3 TB/s: 64 cache lines per load.)
__global__ __launch_bounds__(256) void chain_transpose_kernel(const float* __restrict__ X, int64_t ldx, int64_t r0,
                                                              int64_t steps, int64_t ldc, float* __restrict__ Xc,
                                                              const WaveRuns runs) {
  __shared__ __attribute__((aligned(16))) float t[4 * 8 * TROW];
  const int k = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  if (q >= runs.pre[runs.n]) return;  // the whole wave (no workgroup barrier below)
  int r = 0;
  while (q >= runs.pre[r + 1]) ++r;
  const int64_t s0 = (runs.w0[r] + q - runs.pre[r]) * TW;
  const int nv = (int)(steps - s0 < TW ? steps - s0 : TW);
  const float* src = X + (int64_t)k * ldx + 8 * (r0 + s0);
  float* tw = t + wave * 8 * TROW;
  const int h = lane & 1, sl = lane >> 1;
  f32x4 v[8];
  if (nv == TW) {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src) + 64 * q + lane);
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      v[q] = 32 * q + sl < nv ? reinterpret_cast<const f32x4*>(src)[64 * q + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) tw[(4 * h + e) * TROW + 32 * q + sl] = v[q][e];
  // same wave: its LDS ops complete in order; the clobber keeps the compiler
  // from moving the reads above the writes
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float* dst = Xc + (int64_t)k * 8 * ldc + s0 + 4 * lane;
  if (nv == TW) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      *reinterpret_cast<f32x4*>(dst + (int64_t)c * ldc) = *reinterpret_cast<const f32x4*>(tw + c * TROW + 4 * lane);
  } else {
    for (int c = 0; c < 8; ++c)
      for (int e = 0; e < 4 && 4 * lane + e < nv; ++e) dst[(int64_t)c * ldc + e] = tw[c * TROW + 4 * lane + e];
  }
}

// The tap-major blocks of a training-order client matrix (a convolution
// weight stored [KK][Cin][Cout], KK = kh * kw, whose reference order is
// torch's [Cout][Cin][KK]): chain_transpose_kernel skips them, this kernel
// writes their coordinates chain-major.  A workgroup takes a tile of 32 output
// channels x CI input channels x every tap of one row: coalesced 128-B reads of
// the training layout (32 channels of one (tap, input channel)) into LDS, then,
// per output channel, its run of CI * KK consecutive torch coordinates written
// chain-major (chain c = u % 8, step u / 8 - r0: CI * KK / 8 consecutive floats
// per chain).  The next CI of the same channels continues those runs: tiles
// are numbered channel-group-major and dealt to the XCDs in contiguous ranges
// (blockIdx % 8 is the XCD), so the workgroups that fill one stretch of a chain
// stream share an L2 and run together.  Grid (tiles, K).
// the dense write enumeration divides item indices < TAP_CO * TAP_ROWS through
// a float reciprocal: exact while they stay far below 2^24 / (the divisor)
static_assert(TAP_CO * TAP_ROWS < (1 << 14), "dense write items exact in fp32");

// CMP: a dead region's compact form (dp): the tile holds the live taps alone,
// TAP_ROWS / nl input channels of each, so that an output channel's run stays
// as long in the live stream as a whole block's run is in the plain one
template <int KKT, bool VEC, bool CMP = false>  // KKT: 9, 1, or 0 = KK at run time; VEC: 16-B aligned tile rows
__global__ __launch_bounds__(256) void tap_chain_kernel(const float* __restrict__ X, int64_t ldx, int64_t off,
                                                        int Cout, int Cin, int KKr, int64_t r0, int64_t steps,
                                                        int64_t ldc, float* __restrict__ Xc,
                                                        const float* __restrict__ gdead, uint64_t dead, int nneg,
                                                        const DeadPlan dp) {
  constexpr int TCO = TAP_CO, TROWS = TAP_ROWS;
  __shared__ float tile[TROWS][TCO + 1];
  const int KK = KKT > 0 ? KKT : KKr;
  const int NR = CMP ? dp.nl : KK;  // tile rows per input channel: the taps it holds
  const int CI = TROWS / NR;
  const int nci_t = (Cin + CI - 1) / CI, ntiles = (int)gridDim.x;
  // XCD-contiguous tile numbering: XCD x = blockIdx % 8 takes tiles
  // [x * ntiles / 8, (x + 1) * ntiles / 8)
  const int x = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
  const int tl = x * (ntiles / 8) + min(x, ntiles % 8) + j;
  const int co0 = (tl / nci_t) * TCO, ci0 = (tl % nci_t) * CI;
  const int nci = min(CI, Cin - ci0), nco_v = min(TCO, Cout - co0);
  const int k = blockIdx.y;
  const float* row = X + (int64_t)k * ldx + off;
  // dead taps (flr_pairwise_l2_reference_tap_dead): read from the global
  // vector at the same offset, negated on the sign-flipped rows
  const float* grow = gdead ? gdead + off : row;
  const float gs = k < nneg ? -1.f : 1.f;
  auto is_dead = [&](int t) { return t < 64 && ((dead >> t) & 1); };
  auto src = [&](int t) { return is_dead(t) ? grow : row; };
  auto sgn = [&](int t) { return is_dead(t) ? gs : 1.f; };  // (x * 1 == x, -x exact)
  const int nrows = NR * CI;
  auto tap_of = [&](int tr) { return CMP ? dead_nib(dp.tap, tr) : tr; };  // tile row group tr's tap
  // load: tile row r = t * CI + ci, column = output channel; every load of a
  // thread issued before its LDS stores
  if constexpr (VEC) {  // nco_v == TCO: a row is TCO / 4 pieces of 16 B
    constexpr int LPR = TCO / 4, RPP = 256 / LPR;  // lanes per row, rows per pass
    const int sub = threadIdx.x % LPR, rr = threadIdx.x / LPR;
    constexpr int IT = (TROWS + RPP - 1) / RPP;
    f32x4 v[IT];
#pragma unroll
    for (int q = 0; q < IT; ++q) {
      const int r = rr + RPP * q, tr = r / CI, ci = r - tr * CI, t = tap_of(tr);
      const int64_t e = ((int64_t)t * Cin + ci0 + ci) * Cout + co0 + 4 * sub;
      if (!(r < nrows && ci < nci))
        v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      else if (!CMP && is_dead(t))  // the global vector, re-read by every client: cached loads
        v[q] = *reinterpret_cast<const f32x4*>(grow + e) * gs;
      else
        v[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + e));
    }
#pragma unroll
    for (int q = 0; q < IT; ++q) {
      const int r = rr + RPP * q;
      if (r < nrows)
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r][4 * sub + e] = v[q][e];
    }
  } else {
    for (int e = threadIdx.x; e < nrows * TCO; e += 256) {
      const int co = e % TCO, r = e / TCO, t = tap_of(r / CI), ci = r % CI;
      if (ci < nci && co < nco_v)
        tile[r][co] = (CMP ? row : src(t))[((int64_t)t * Cin + ci0 + ci) * Cout + co0 + co] * (CMP ? 1.f : sgn(t));
    }
  }
  __syncthreads();
  if constexpr (CMP) {
    // the live coordinates alone, at their slots of the live stream (Xc: the
    // region's streams): output channel co's items (ci, live tap), tap
    // fastest, dealt to the lanes with a stride of 8 — with one live tap a
    // chain's coordinates are 8 input channels apart, so consecutive lanes
    // write consecutive slots of one chain
    const int per = nci * dp.nl, n = nco_v * per, p8 = per / 8;
    const bool deal = per % 8 == 0;
    float* outl = Xc + (int64_t)k * 8 * ldc;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int co = i / per, l = i - co * per, q = deal ? 8 * (l % p8) + l / p8 : l;
      const int ci = q / dp.nl, lt = q - ci * dp.nl, t = dead_nib(dp.tap, lt);
      const int64_t rel = ((int64_t)(co0 + co) * Cin + ci0 + ci) * KK + t;
      outl[(rel & 7) * ldc + dead_slot(rel, t, dp.nl, dp.rank)] = tile[lt * CI + ci][co];
    }
    return;
  }
  // write: output channel co's run [u0, u0 + nci * KK) (at most 288
  // coordinates: 38 steps per chain), clipped to the segment
  // [8 r0, 8 (r0 + steps)), chain-major: a wave writes consecutive steps of
  // a chain stream
  const int64_t L = (int64_t)nci * KK;
  const int64_t ulo = 8 * r0, uhi = 8 * (r0 + steps);
  float* out = Xc + (int64_t)k * 8 * ldc;
  {
    // every co's run whole inside the segment, and the same chain split for
    // every co (Cin KK and L multiples of 8: m steps per chain): the items
    // enumerated densely, (co, chain, step) with step fastest — every lane
    // busy, against 36 or 37 of 64 in the general loop below (-13 % time)
    const int64_t CL = (int64_t)Cin * KK;
    const int64_t ufirst = off + ((int64_t)co0 * Cin + ci0) * KK;
    if (CL % 8 == 0 && L % 8 == 0 && ufirst >= ulo && ufirst + (nco_v - 1) * CL + L <= uhi) {
      const int Li = (int)L, m = Li / 8, a0 = (int)(ufirst & 7);
      const int64_t sb0 = (ufirst >> 3) - r0, CLs = CL / 8;
      const float inv_L = 1.f / (float)Li, inv_m = 1.f / (float)m;
      const int n = nco_v * Li;
#pragma unroll 4
      for (int i = threadIdx.x; i < n; i += 256) {
        const int co = (int)(((float)i + 0.5f) * inv_L);  // exact: i < 2^14
        const int q = i - co * Li;
        const int c = (int)(((float)q + 0.5f) * inv_m);
        const int jj = q - c * m;
        const int dc = (c - a0) & 7;  // chain c's first coordinate in the run: u0 + dc
        const int rel = dc + 8 * jj, ci = rel / KK, t = rel - ci * KK;
        out[(int64_t)c * ldc + sb0 + co * CLs + ((a0 + dc) >> 3) + jj] = tile[t * CI + ci][co];
      }
      return;
    }
  }
  // the general tile (ragged, or crossing a segment end): item i -> (co =
  // i / 512, chain = i / 64 % 8, step slot i % 64)
  static_assert(TROWS / 8 + 1 <= 64, "a run's steps fit its slots");
#pragma unroll 4
  for (int i = threadIdx.x; i < nco_v * 512; i += 256) {
    const int ns = i & 63, c = (i >> 6) & 7, co = i >> 9;
    const int64_t u0 = off + ((int64_t)(co0 + co) * Cin + ci0) * KK;
    const int64_t u = 8 * ((u0 >> 3) + ns) + c;
    if (u >= u0 && u < u0 + L && u >= ulo && u < uhi) {
      const int rel = (int)(u - u0), ci = rel / KK, t = rel - ci * KK;
      out[(int64_t)c * ldc + ((u >> 3) - r0)] = tile[t * CI + ci][co];
    }
  }
}

// The slots of a region's streams that no step fills, zeroed: [0, n0) and
// [z0, z1) of stream blockIdx.x (one launch: a pair of 2-D memsets cost more on
// the host than the kernels they start)
__global__ __launch_bounds__(256) void zero_slots_kernel(float* __restrict__ Xc, int64_t ldc, int n0, int64_t z0,
                                                         int64_t z1) {
  float* row = Xc + (int64_t)blockIdx.x * ldc;
  const int n = n0 + (int)(z1 - z0);
  for (int i = threadIdx.x; i < n; i += 256) row[i < n0 ? i : z0 + (i - n0)] = 0.f;
}

// The dead stream of a block (DeadPlan), once per call: T = g + g at every dead
// coordinate's slot, and *flag raised where a dead value of g is not finite
// (the same-kind pairs' inf - inf, which skipping their dead steps would miss:
// ref_finish_kernel).  T is zeroed before.  Item -> (co, ci, dead tap), tap fastest.
__global__ __launch_bounds__(256) void dead_stream_kernel(const float* __restrict__ g, int64_t off, int Cout, int Cin,
                                                          const DeadPlan dp, int64_t ldt, float* __restrict__ T,
                                                          int* __restrict__ flag) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)Cout * Cin * dp.nd) return;
  const int64_t q = idx / dp.nd;
  const int t = dead_nib(dp.tap, (int)(idx - q * dp.nd));
  const int64_t co = q / Cin, ci = q - co * Cin;
  const float v = g[off + ((int64_t)t * Cin + ci) * Cout + co];
  if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) *flag = 1;
  const int64_t rel = q * 9 + t;
  T[(rel & 7) * ldt + dead_slot(rel, t, dp.nd, dp.rank)] = v + v;
}

// The throughput forms' operand layout (agg_pairwise_ref_quad.hip).
// Xq tile: rows k0 .. k0 + 15 x blocks b0 .. b0 + 15 (64 steps = 512 coordinates
// = 2 KB of each row): coalesced 1-KB row reads into LDS, then thread (k, block)
// takes its row's 32 coordinates of the block and stores 8 chain pieces (16 B:
// 4 steps each), 256-B runs of consecutive rows.  Steps past `steps` are 0.
__global__ __launch_bounds__(256) void quad_transpose_kernel(const float* __restrict__ X, int64_t ldx, int K,
                                                             int64_t r0, int64_t steps, int64_t NB, int64_t Kp,
                                                             float* __restrict__ Xq) {
  __shared__ f32x4 t[QTB][QTB * 8 + 1];
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * QTB;
  const int k0 = blockIdx.y * QTB;
  const int64_t u0 = 8 * (r0 + 4 * b0), uend = 8 * (r0 + steps);  // this tile's first coordinate, the segment's end
  f32x4 v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int idx = q * 256 + tid, row = idx >> 7, p = idx & 127;
    const int64_t u = u0 + 4 * p;
    v[q] = (k0 + row < K && u < uend)
               ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(X + (int64_t)(k0 + row) * ldx + u))
               : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int idx = q * 256 + tid;
    t[idx >> 7][idx & 127] = v[q];
  }
  __syncthreads();
  const int k = tid & 15, bl = tid >> 4;
  if (k0 + k >= K) return;  // rows past K: never a valid pair's operand
  f32x4 w[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) w[q] = t[k][8 * bl + q];
  // coordinate 32 bl + 4 q + m = 8 (4 bl + e) + c: step e = q / 2, chain c = 4 (q % 2) + m
  float* out = Xq + ((b0 + bl) * Kp + k0 + k) * 4;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int h = c >> 2, m = c & 3;
    *reinterpret_cast<f32x4*>(out + (int64_t)c * NB * Kp * 4) = f32x4{w[h][m], w[2 + h][m], w[4 + h][m], w[6 + h][m]};
  }
}

int launch_chain_transpose(const float* X, int64_t K, int64_t ldx, int64_t r0, int64_t steps, int64_t ldc, float* Xc,
                           const WaveRuns& runs, hipStream_t st) {
  const int64_t nw = runs.pre[runs.n];
  if (nw == 0) return FLR_OK;
  hipLaunchKernelGGL(chain_transpose_kernel, dim3((unsigned)((nw + 3) / 4), (unsigned)K), dim3(256), 0, st, X, ldx, r0,
                     steps, ldc, Xc, runs);
  return launch_status("chain_transpose_kernel");
}

// rows: the tile rows an input channel takes (its taps: KK, or the live ones)
static unsigned tap_tiles(const TapBlock& tb, int64_t rows) {
  const int64_t cit = TAP_ROWS / rows;  // input channels per tile
  return (unsigned)((tb.co + TAP_CO - 1) / TAP_CO * ((tb.ci + cit - 1) / cit));
}
// 16-B aligned rows, full 32-channel tiles
static bool tap_vec(const TapBlock& tb) { return tb.off % 4 == 0 && tb.co % TAP_CO == 0; }

int launch_tap_chain(const float* X, int64_t K, int64_t ldx, const TapBlock& tb, int64_t r0, int64_t steps, int64_t ldc,
                     float* Xc, const float* gdead, uint64_t dead, int nneg, hipStream_t st) {
  const bool vec = tap_vec(tb);
  auto kern = tb.kk == 9 ? (vec ? tap_chain_kernel<9, true> : tap_chain_kernel<9, false>)
            : tb.kk == 1 ? (vec ? tap_chain_kernel<1, true> : tap_chain_kernel<1, false>)
                         : (vec ? tap_chain_kernel<0, true> : tap_chain_kernel<0, false>);
  hipLaunchKernelGGL(kern, dim3(tap_tiles(tb, tb.kk), (unsigned)K), dim3(256), 0, st, X, ldx, tb.off, (int)tb.co,
                     (int)tb.ci, (int)tb.kk, r0, steps, ldc, Xc, dead ? gdead : nullptr, dead, nneg, DeadPlan{});
  return launch_status("tap_chain_kernel");
}

int launch_tap_chain_live(const float* X, int64_t K, int64_t ldx, const TapBlock& tb, int64_t r0, int64_t steps,
                          int64_t ldc, float* Xc, uint64_t dead, int nneg, const DeadPlan& live, hipStream_t st) {
  auto kern = tap_vec(tb) ? tap_chain_kernel<9, true, true> : tap_chain_kernel<9, false, true>;
  hipLaunchKernelGGL(kern, dim3(tap_tiles(tb, live.nl), (unsigned)K), dim3(256), 0, st, X, ldx, tb.off, (int)tb.co,
                     (int)tb.ci, 9, r0, steps, ldc, Xc, (const float*)nullptr, dead, nneg, live);
  return launch_status("tap_chain_kernel");
}

int launch_zero_slots(float* Xc, int64_t ldc, int64_t K, int n0, int64_t z0, int64_t z1, hipStream_t st) {
  hipLaunchKernelGGL(zero_slots_kernel, dim3((unsigned)(K * 8)), dim3(256), 0, st, Xc, ldc, n0, z0, z1);
  return launch_status("zero_slots_kernel");
}

int launch_dead_stream(const float* g, const TapBlock& tb, const DeadPlan& deadp, int64_t ldt, float* T, int* flag,
                       hipStream_t st) {
  const int64_t n = tb.co * tb.ci * deadp.nd;
  hipLaunchKernelGGL(dead_stream_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, tb.off, (int)tb.co,
                     (int)tb.ci, deadp, ldt, T, flag);
  return launch_status("dead_stream_kernel");
}

int launch_quad_transpose(const float* X, int64_t ldx, int64_t K, int64_t r0, int64_t steps, int64_t NB, int64_t Kp,
                          float* Xq, hipStream_t st) {
  hipLaunchKernelGGL(quad_transpose_kernel, dim3((unsigned)(NB / QTB), (unsigned)((K + QTB - 1) / QTB)), dim3(256), 0,
                     st, X, ldx, (int)K, r0, steps, NB, Kp, Xq);
  return launch_status("quad_transpose_kernel");
}

}  // namespace pwref
}  // namespace flr
