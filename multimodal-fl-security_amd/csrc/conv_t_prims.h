// a2 — client-batched convolution with TAP-MAJOR weights, the training
// engine's layout for every conv whose channel counts are multiples of 64
// (all of ResNet-18 but the stem).  Same products as train_conv.hip
// (nn.Conv2d(bias=False) of the conv blocks, src/models/cub200_cnn.py:71-77
// template; trained per client in run_experiments.py:216-235), with the
// weights of client k stored as W_t[k][kh][kw][Cin][Cout] instead of torch's
// [Cout][Cin][kh][kw].  The trainer converts at the round boundaries
// (load_global / export); inside the round nothing else sees the layout.
//
// Why: at a fixed kernel tap the weight slab is a plain [Cin][Cout] matrix, so
//   fwd   A(m = co, k = ci) is contiguous along m -> 16-B loads, [k][m] LDS image
//   dgrad A(m = ci, k = co) is contiguous along k -> 16-B loads, [m][k] LDS image
//   wgrad writes C(m = ci, n = co) with coalesced rows.
// The activation operand is an im2col gather; it uses raw buffer loads whose
// per-element stride sits in soffset (an SGPR) and whose padding taps carry an
// out-of-range voffset (the hardware returns 0), so a gathered element costs
// no VALU work — f32 MFMA shares the VALU's issue rate on gfx950, so address
// arithmetic comes straight out of matrix throughput.
//
// Tiles: 64 x 64 outputs per workgroup, 32-deep K-tiles (one kernel tap each:
// C % 64 == 0), 4 waves of 32 x 32, v_mfma_f32_32x32x2_f32; MFMA (j, t) of a
// K-tile feeds reduction index 8j + 4h + t from lane half h, so an operand
// held as [row][k] is read with one ds_read_b128 per four MFMAs and one held
// as [k][row] with ds_read_b32.  Register-staged one K-tile ahead, double-
// buffered LDS, deterministic split-K for long reductions (partials reduced
// in split order).
//
// The code lives in seven headers and five translation units:
//   bf16x6.h           buffer loads, the bf16 split, the six-product order (shared
//                      with train_gru.hip and train_stem.hip)
//   conv_t_prims.h     (this file) tile constants, fp32 LDS images, knobs
//   conv_t_plans.h     the load plans: FwdT, DgradT, WgtT, Dense*, Stem*, BGemm
//   conv_t_kernels.h   the epilogue and the GEMM kernels
//   conv_t_dgrad_fused.h  the fused strided data gradient (sgemm_body's K-loop per parity class)
//   conv_t_launch.h    the launch policy (form, tile, split-K: resolve) and launch
//   conv_t_ablation.h  the measured-slower and timing-only forms (make ABLATION=1 only)
//   train_conv_t_{im2col,fwd,dgrad,wgrad,bgemm}.hip   the extern "C" entry points;
//   each unit instantiates only the kernels its entry points launch.
#pragma once

#include "bf16x6.h"
#include "conv_common.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace flr {
namespace convt {

using conv::Geom;
using conv::udiv;

constexpr int BM = 64, BN = 64, BK = 32, THREADS = 256;
constexpr int SKR = 68;  // [k][row] image row stride (floats)
constexpr int SRK = 36;  // [row][k] image row stride
constexpr int TILE = 64 * SRK;

enum Lay { KR_VEC = 0, KR_GATHER = 1, RK_VEC = 2, RK_GATHER = 3 };

// ---- LDS images -------------------------------------------------------------
template <int LAY>
__device__ __forceinline__ void stash(float* buf, const float (&v)[8], int tid) {
  if constexpr (LAY == KR_VEC) {  // thread: 4 rows (tid % 16), k = tid / 16 + 16 i
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<f32x4*>(buf + (tid / 16 + 16 * i) * SKR + 4 * (tid % 16)) =
          f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
  } else if constexpr (LAY == KR_GATHER) {  // row tid % 64, k = tid / 64 + 4 i
#pragma unroll
    for (int i = 0; i < 8; ++i) buf[(tid / 64 + 4 * i) * SKR + tid % 64] = v[i];
  } else if constexpr (LAY == RK_VEC) {  // row tid / 8 + 32 i, k = 4 (tid % 8) .. +3
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<f32x4*>(buf + (tid / 8 + 32 * i) * SRK + 4 * (tid % 8)) =
          f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
  } else {  // RK_GATHER: row tid / 32 + 8 i, k = tid % 32
#pragma unroll
    for (int i = 0; i < 8; ++i) buf[(tid / 32 + 8 * i) * SRK + tid % 32] = v[i];
  }
}

// Operand values of MFMAs (j, 0..3) for this lane: k = 8j + 4h + t, row = rb.
template <int LAY>
__device__ __forceinline__ f32x4 frag(const float* buf, int rb, int j, int h) {
  if constexpr (LAY == RK_VEC || LAY == RK_GATHER) {
    return *reinterpret_cast<const f32x4*>(buf + rb * SRK + 8 * j + 4 * h);
  } else {
    const float* p = buf + (8 * j + 4 * h) * SKR + rb;
    return f32x4{p[0], p[SKR], p[2 * SKR], p[3 * SKR]};
  }
}

// ---- the bf16x6 MFMA form (bf16x6.h) on fp32 images ----------------------------
// The LDS images stay fp32; each wave splits the eight values of its fragment:
// lane (l32, h) supplies row l32 and reduction indices k0 .. k0+7, k0 = 16 s + 8 h.
template <int LAY>
__device__ __forceinline__ void frag8(const float* buf, int rb, int k0, float (&v)[8]) {
  if constexpr (LAY == RK_VEC || LAY == RK_GATHER) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(buf + rb * SRK + k0);
    const f32x4 b = *reinterpret_cast<const f32x4*>(buf + rb * SRK + k0 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = a[e];
      v[4 + e] = b[e];
    }
  } else {
    const float* p = buf + k0 * SKR + rb;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = p[e * SKR];
  }
}

// FLR_GEMM=f32 selects the exact-f32 MFMA (A/B timing, cross-checks); read per
// launch so one process can compare both forms.
// FLR_XCD=0 turns the XCD-aware tile order off (A/B timing).
// bit 0: the XCD-aware tile order; A/B (split-at-stash kernels): bits 8-15
// FLR_GEMM_STAGGER = n, workgroups of odd XCD slot start n x 512 cycles late;
// bit 16 FLR_GEMM_SPRIO=1, those workgroups at s_setprio 1 for the whole loop
inline int xcd_remap() {
  int r = knob_off("FLR_XCD") ? 0 : 1;
  const char* st = flr::knob("FLR_GEMM_STAGGER");
  if (st) r |= (std::min(255, std::max(0, atoi(st))) << 8);
  if (knob_on("FLR_GEMM_SPRIO")) r |= 1 << 16;
  return r;
}
// the A/B controls above, at the start of a split-at-stash kernel
__device__ __forceinline__ void odd_slot_controls(int remap) {
  const int lid = (int)blockIdx.x + (int)gridDim.x * ((int)blockIdx.y + (int)gridDim.y * (int)blockIdx.z);
  if (((lid >> 3) & 1) == 0) return;
  if ((remap >> 16) & 1) __builtin_amdgcn_s_setprio(1);
  for (int i = (remap >> 8) & 255; i > 0; --i) __builtin_amdgcn_s_sleep(8);
}

// Wave priority raised around each MFMA cluster (FLR_PRIO=0: off, for A/B).
inline int mfma_prio() {  // measured +0-5 % on the encoder GEMMs and the 3x3 convs (FLR_PRIO=0 turns it off)
  return knob_off("FLR_PRIO") ? 0 : 1;
}

// 0: exact f32 MFMA; 2: bf16x6, product-major, software-pipelined; 5 (default):
// split at stash time where the plan supports it (fwd / dgrad / batched GEMM),
// else 2.  FLR_GEMM=f32 | pipe | stash.  The tools build (make ABLATION=1) adds
// the measured-slower forms 1 (accumulator-chain order, FLR_GEMM=chain) and 4
// (the unpipelined loop, =old), and the wrong-result timing ablation 3 (=A).
inline int gemm_form() {
  const char* e = flr::knob("FLR_GEMM");
  if (e && e[0] == 'f') return 0;
#ifdef FLR_ABLATION
  if (e && e[0] == 'c') return 1;
  if (e && e[0] == 'A') return 3;  // ablation (timing only, wrong results): one bf16 term, no split; tools build only
  if (e && e[0] == 'o') return 4;  // the unpipelined product-major loop (A/B timing)
#endif
  if (e && e[0] == 'p') return 2;  // the pipelined loop for every plan
  return 5;  // split at stash (bf16 LDS images) where the plan has k8 loads, else pipelined
}

// ---- load plans ---------------------------------------------------------------
// Tap of a reduction slot: W_t offset of (tap, 0, 0) = tap_index * Cin * Cout.
// (kh, kw) of a tile-uniform reduction slot, by rectangle arithmetic (the host
// accepts only geometries whose live taps form a rectangle: args_ok)
__device__ __forceinline__ void slot_tap(const Geom& g, int slot, int& kh, int& kw) {
  conv::rect_tap(g.rect, slot, kh, kw);
}
__device__ __forceinline__ int tap_index(const Geom& g, int slot) {
  int kh, kw;
  slot_tap(g, slot, kh, kw);
  return kh * g.KW + kw;
}
// Tile-uniform values the compiler cannot prove uniform (the tap table is
// indexed by a computed slot): broadcast so they live in SGPRs and the buffer
// loads that take them as soffset need no waterfall loop.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Split-at-stash forms (sgemm_body): the thread that loads 8 consecutive k of
// one operand row stashes them as bf16x8.  Row-contiguous operands put the 64
// lanes of a wave on 64 consecutive rows (coalesced along the row); a
// k-contiguous operand instead puts 4 lanes on each row (QUAD: row tid / 4,
// k 8 (tid % 4)), so a wave's load covers 16 rows x 128 B instead of 64 rows x
// 32 B (64 cache lines per instruction).
template <bool QUAD> __device__ __forceinline__ int stash_row(int tid) { return QUAD ? tid >> 2 : tid & 63; }
template <bool QUAD> __device__ __forceinline__ int stash_k(int tid) { return QUAD ? 8 * (tid & 3) : 8 * (tid >> 6); }

}  // namespace convt
}  // namespace flr
