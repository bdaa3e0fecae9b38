// The launch policy of the tap-major GEMM engine: which kernel form one launch
// of a plan runs, on which workgroup tile, with how many split-K parts.
// resolve() decides it, once; launch() runs what resolve() says, and every
// query (workspace refusals, clip-norm slots, the resident probes, the fused
// data gradient's per-class split counts) reads the same resolved value.  A new
// kernel form is added to resolve() and to launch()'s dispatch, nowhere else.
#pragma once

#include "conv_t_kernels.h"

#include <climits>

namespace flr {
namespace convt {

// Split-K count from the PER-CLIENT problem only (never the client count K):
// a client's reduction order — and so its trained weights — must not depend
// on how many clients share its GPU (bit-identical results at 1/2/4/8 GPUs).
// 16 tiles per client = the 2048-workgroup target at the nominal 128 clients.
// sub: sub-tiles per workgroup tile; min_kt: fewest K-tiles a split may keep.
inline int choose_splits(int M, int N, int R, int sub, int min_kt) {
  const int tiles = cdiv(M, BM) * cdiv(N, BN) / sub;
  const int ktiles = cdiv(R, BK);
  int S = 1;
  while (S < 16 && tiles * S < 16 && ktiles / (2 * S) >= min_kt) S *= 2;
  return S;
}

// Fewest K-tiles per split-K part.  Convolutions: 32 (measured per layer against
// 8 and 16, tools/conv_bench.py): a workgroup's unhidden prologue (first load,
// split, barrier) amortises over more K-tiles; the l3b / l4 forward and dgrad
// gain the most.  Batched GEMMs: 32 (8 cost 1.7 ms per C3 round in split-K
// partials and reduce passes).  A strided dgrad's parity class has few tiles per
// client (l3a: one 128 x 128 tile): it keeps the deeper split-K of 8, or the
// launch runs ~128 workgroups on 256 CUs.  These set the reduction order, hence
// the trained bits: constants, not switches.
constexpr int MIN_KT = 32, MIN_KT_STRIDED_DGRAD = 8;
template <class Plan>
inline int plan_min_kt(const Plan& pl) {
  if constexpr (std::is_same<Plan, DgradT>::value) return pl.g.stride == 1 ? MIN_KT : MIN_KT_STRIDED_DGRAD;
  return MIN_KT;
}

// Split-K partials of K clients' M x N products: enough for any sub-tile count (1, 2, 3, 4).
inline size_t splits_bytes(int M, int N, int R, int64_t K, int min_kt) {
  int S = 1;
  for (int sub : {1, 2, 3, 4}) S = std::max(S, choose_splits(M, N, R, sub, min_kt));
  return S > 1 ? (size_t)S * K * M * N * sizeof(float) : 0;
}
template <class Plan>
size_t splits_bytes(const Plan& pl) {
  return splits_bytes(pl.M(), pl.N(), pl.R(), pl.g.Kc, plan_min_kt(pl));
}

// Tile code 10 * MS + NS.  Besides the square shapes, the tap-major
// convolutions take 64 x 192 / 192 x 64 (13 / 31) and 64 x 256 / 256 x 64
// (14 / 41): a 64-row operand (layer1's 64 channels) then feeds three or four
// MFMA sub-tiles per fragment read instead of one or two (LDS: five sub-tiles
// of bf16 images, still two workgroups per CU).
template <class Plan>
constexpr bool wide_tiles() {
  return std::is_same<Plan, FwdT>::value || std::is_same<Plan, DgradT>::value ||
         std::is_same<Plan, WgtT<true>>::value || std::is_same<Plan, WgtT<false>>::value;
}

// The plan's default workgroup tile: 64 x 64 (MS = NS = 1: 4 waves of 32 x 32,
// 4 workgroups/CU) or 128 x 128 (MS = NS = 2: each wave 64 x 64, its A and B
// fragments — and their bf16 splits — reused twice; 2 workgroups/CU).
// Convolutions, measured per ResNet-18 layer on MI355X (tools/conv_bench.py):
// 128 x 128 wins where both dimensions allow it and the tile still has work — a
// reduction of >= 512 or more than 128 x 512 outputs per client; 64 x 64
// everywhere else.  FLR_CONV_TILE forces any shape that leaves no sub-tile empty
// (A/B, read per launch); a code the plan rejects runs 64 x 64.
// Batched GEMMs: 128 x 128 for the encoder-sized products (M, N >= 128 and a long
// reduction or many outputs), 64 x 64 for the small ones (the GRU recurrence and
// the head, M = batch = 32); partial edge tiles are bounds-checked in the loads
// and stores.  FLR_BGEMM_TILE=11|22 forces it.
template <class Plan>
inline int plan_tile(const Plan& pl) {
  const int M = pl.M(), N = pl.N(), R = pl.R();
  if constexpr (std::is_base_of<BGemmArgs, Plan>::value) {
    const int forced = knob_int("FLR_BGEMM_TILE", 11, 22, 0);
    if (forced == 11 || forced == 22) return forced;
    return (M >= 128 && N >= 128 && (R >= 256 || (int64_t)M * N >= 128 * 512)) ? 22 : 11;
  } else {
    const int forced = knob_int("FLR_CONV_TILE", INT_MIN, INT_MAX, 0);
    int tile = 11;
    if (forced) {
      const int ms = forced / 10, ns = forced % 10;
      const bool ok = ms >= 1 && ns >= 1 && ms * ns <= 4 && (wide_tiles<Plan>() || (ms <= 2 && ns <= 2)) &&
                      M > 64 * (ms - 1) && N > 64 * (ns - 1);
      if (ok) return forced;
    } else if (M % 128 == 0 && N % 128 == 0 && (R >= 512 || (int64_t)M * N > 128 * 512)) {
      tile = 22;
    }
    // dgrad with 64 input channels (layer1): 64 x 128 tiles, the A fragment feeding
    // two B sub-tiles (measured 178 -> 147 us at l1)
    if (std::is_same<Plan, DgradT>::value && tile == 11 && M == 64 && N % 128 == 0) tile = 12;
    return tile;
  }
}

// Narrow-N tiles (sgemm_body NAR) for a conv forward / data gradient whose GEMM has
// at most 32 columns (the l4 layers at 32 x 32 inputs: B * 1 * 1); FLR_CONV_NARROW=0:
// the 64-wide tiles (A/B, read per launch).
inline bool narrow_shape(int M, int N) { return N <= 32 && M % (2 * BM) == 0 && !knob_off("FLR_CONV_NARROW"); }

// The resident-B form (rgemm_kernel): the forward and the stride-1 data gradient of
// a "same" convolution with 64 output rows and 64 reduction channels whose images
// tile 128 columns (layer1 of ResNet-18).  FLR_CONV_RESIDENT=0: off (A/B, read per launch).
template <class Plan>
bool resident_shape(const Plan& pl) {
  const Geom& g = pl.g;
  if (knob_off("FLR_CONV_RESIDENT")) return false;
  if (g.stride != 1 || g.Ho != g.H || g.Wo != g.W) return false;
  if (pl.M() != BM || pl.Cr() != 2 * BK) return false;
  const int hw = g.H * g.W;
  if (hw > RES_N || RES_N % hw != 0) return false;
  return pl.R() >= 2 * pl.Cr();  // one tap: nothing is staged twice
}

// The resident weight gradient (rwgemm_kernel): a stride-1 "same" convolution with
// 64 channels on both sides (one 64 x 64 tile per tap: layer1 of ResNet-18) whose
// images tile the 64-pixel chunk and whose live taps form whole groups of RW_TG.
// FLR_WGRAD_RESIDENT=0: off (A/B, read per launch).
inline bool wgrad_resident_shape(const Geom& g) {
  if (knob_off("FLR_WGRAD_RESIDENT")) return false;
  if (g.stride != 1 || g.Ho != g.H || g.Wo != g.W) return false;
  if (g.Cin != BM || g.Cout != BN) return false;
  if (g.ntaps < 2 || g.ntaps % RW_TG != 0) return false;  // one tap: nothing is staged twice
  return RW_PIX % (g.H * g.W) == 0;
}

// Small client counts (K/G clients per GPU at G = 8: 16 at C3) leave the
// default tiles' grids below one wave of the chip: layer2 / layer3 of ResNet-18
// launch 4 workgroups of 128 x 128 per client.  Forward and data-gradient
// launches whose grid would hold fewer than FILL_WG workgroups then run on
// 64 x 64 tiles with the DEFAULT tile's split-K count: every output element is
// the same K-tile / k-step / product sequence, so the result is bit-identical
// to the default tiles (and the model to the one at G = 1).  The weight
// gradients keep their tiles: their clip-norm partial slots follow the tile.
// FLR_CONV_FILL=0: off (A/B, read per launch).
constexpr int FILL_WG = 512;  // two 128 x 128 workgroups per CU on 256 CUs

// What one launch of a plan is.
enum class Kind { None, Tiles, Narrow, ResidentB, ResidentW };
struct Launch {
  Kind kind = Kind::None;  // None: nothing to compute (an empty reduction)
  int ms = 1, ns = 1;      // the tile the kernel is instantiated for
  int sub = 1;             // the sub-tile count S was chosen for (the default tile's under fill)
  int S = 1;               // split-K parts, after the workspace check
  bool ws_short = false;   // S fell to 1 because the workspace cannot hold the partials
  dim3 grid;
  int sq_slots = 0;        // weight gradients: clip-norm partial slots per client the launch writes
};

// Precedence: the resident weight gradient, the resident-B form, the narrow tiles
// (on 64 x 64 fill tiles when their grid is under half a wave of the chip), the
// fill tiles, the plan's default tile.  Every form that replaces the default tile
// keeps the split count of the tile it replaces, so each form's bits are the
// default path's.  The resident-B form needs a split count of 1 and so ignores
// the workspace.
template <class Plan>
Launch resolve(const Plan& pl, const void* ws, size_t ws_bytes) {
  constexpr bool dgrad = std::is_same<Plan, DgradT>::value, fd = dgrad || std::is_same<Plan, FwdT>::value;
  Launch L;
  const int M = pl.M(), N = pl.N(), R = pl.R(), K = pl.g.Kc;
  if (R == 0 && !dgrad) return L;  // a dgrad class with no tap stores zeros
  const bool stash = gemm_form() == 5;
  const int tile = plan_tile(pl), min_kt = plan_min_kt(pl);
  L.kind = Kind::Tiles;
  L.ms = tile / 10;
  L.ns = tile % 10;
  L.sub = L.ms * L.ns;
  L.S = choose_splits(M, N, R, L.sub, min_kt);
  if constexpr (std::is_same<Plan, WgtT<true>>::value) {  // H W % 4 != 0 (WgtT<false>) keeps the default kernel
    if (stash && tile == 11 && wgrad_resident_shape(pl.g)) L.kind = Kind::ResidentW;
  }
  if constexpr (fd) {
    const bool fill = !knob_off("FLR_CONV_FILL");
    if (stash && L.S == 1 && resident_shape(pl)) {
      L.kind = Kind::ResidentB;
    } else if (stash && R > 0 && narrow_shape(M, N)) {
      L.sub = 2;
      L.S = choose_splits(M, N, R, 2, min_kt);
      // under one wave of the chip (few clients per GPU): the 64 x 64 tiles with the
      // narrow tiles' split count — twice the workgroups, the same bits
      const bool filled = fill && (int64_t)K * cdiv(M, 2 * BM) * L.S < FILL_WG / 2;
      L.kind = filled ? Kind::Tiles : Kind::Narrow;
      L.ms = filled ? 1 : 2;
      L.ns = 1;
    } else if (fill && L.sub > 1 && (int64_t)K * cdiv(M, BM * L.ms) * cdiv(N, BN * L.ns) * L.S < FILL_WG) {
      L.ms = L.ns = 1;
    }
  }
  if (L.S > 1 && (!ws || ws_bytes < (size_t)L.S * K * M * N * sizeof(float))) {
    L.S = 1;
    L.ws_short = true;
  }
  if (L.kind == Kind::ResidentB) {
    L.grid = dim3((unsigned)cdiv(N, RES_N), 1u, (unsigned)K);
  } else if (L.kind == Kind::ResidentW) {
    L.grid = dim3(1u, (unsigned)(M / BM / RW_TG), (unsigned)(K * L.S));  // M / BM taps (Cin = BM), RW_TG per workgroup
  } else {
    L.grid = dim3((unsigned)cdiv(N, BN * L.ns), (unsigned)cdiv(M, BM * L.ms), (unsigned)(K * L.S));
  }
  // the tile count at split-K 1 (the resident form: one 64 x 64 tile per tap, the
  // same count), else one slot per 256-value treduce block
  if constexpr (has_sq<Plan>::value)
    L.sq_slots = L.S == 1 ? cdiv(N, BN * L.ns) * cdiv(M, BM * L.ms) : (int)(((int64_t)M * N + 255) / 256);
  return L;
}

// The slots a clip-norm launch writes given a workspace of splits_bytes(pl).
template <class Plan>
int sq_slots(const Plan& pl) {
  return resolve(pl, &pl, SIZE_MAX).sq_slots;
}
template <class Plan>
bool resident_ok(const Plan& pl) {
  return resolve(pl, nullptr, 0).kind == Kind::ResidentB;
}
template <class Plan>
bool wgrad_resident_ok(const Plan& pl) {
  return resolve(pl, nullptr, 0).kind == Kind::ResidentW;
}

// The launch's status; with split-K, the reduce pass over its partials.
template <class Plan>
int reduce_splits(const Plan& pl, int S, const float* part, hipStream_t st, const char* name) {
  const int rc = launch_status(name);
  if (rc != FLR_OK || S == 1) return rc;
  const int64_t mn = (int64_t)pl.M() * pl.N();
  hipLaunchKernelGGL(treduce_kernel<Plan>, dim3((unsigned)((mn + 255) / 256), (unsigned)pl.g.Kc), dim3(256), 0, st, pl,
                     S, part);
  return launch_status(name);
}

template <class Plan, int MS, int NS>
int launch_tiles(const Plan& pl, const Launch& L, void* ws, size_t ws_bytes, hipStream_t st, const char* name) {
  const int S = L.S, form = gemm_form();
  float* part = static_cast<float*>(ws);
  float* partp = part;  // where treduce reads (after the planes in the tools build's pre-split form)
  bool done = false;
#ifdef FLR_ABLATION  // the measured-slower and timing-only forms: tools build only
  done = launch_ablation<Plan, MS, NS>(pl, L.grid, S, form, ws, ws_bytes, st, partp);
#endif
  // every form keeps each accumulator's product order: results do not depend on it
  if constexpr (has_k8<Plan>::value) {
    if (!done && form == 5) {
      hipLaunchKernelGGL((sgemm_kernel<Plan, MS, NS>), L.grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap());
      done = true;
    }
  }
  if constexpr (std::is_same<Plan, WgtT<true>>::value && MS == 1 && NS == 1) {
    if (!done && L.kind == Kind::ResidentW) {  // the default kernel's split count, partials and treduce pass
      hipLaunchKernelGGL((rwgemm_kernel<Plan, RW_TG>), L.grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap());
      done = true;
    }
  }
  if constexpr (std::is_same<Plan, WgtT<true>>::value || std::is_same<Plan, WgtT<false>>::value) {
    if (!done && form == 5) {
      hipLaunchKernelGGL((wsgemm_kernel<Plan, MS, NS, true, true>), L.grid, dim3(THREADS), 0, st, pl, S, part,
                         xcd_remap());
      done = true;
    }
  }
  if (!done && form == 0) {
    hipLaunchKernelGGL((tgemm_kernel<Plan, MS, NS, 0>), L.grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap(),
                       mfma_prio());
  } else if (!done) {  // the pipelined loop: asked for, or a plan without k8 loads
    hipLaunchKernelGGL((tgemm_kernel<Plan, MS, NS, 2>), L.grid, dim3(THREADS), 0, st, pl, S, part, xcd_remap(),
                       mfma_prio());
  }
  return reduce_splits(pl, S, partp, st, name);
}

template <class Plan>
int launch(const Plan& pl, void* ws, size_t ws_bytes, hipStream_t st, const char* name) {
  const Launch L = resolve(pl, ws, ws_bytes);
  // a clip-norm launch must write the slots sq_slots() promised: no silent fallback
  if constexpr (has_sq<Plan>::value) {
    if (pl.sq && L.ws_short) return FLR_ERR_WORKSPACE;
  }
  if (L.kind == Kind::None) return FLR_OK;
  if constexpr (std::is_same<Plan, FwdT>::value || std::is_same<Plan, DgradT>::value) {
    if (L.kind == Kind::ResidentB) {
      hipLaunchKernelGGL((rgemm_kernel<Plan>), L.grid, dim3(THREADS), 0, st, pl, xcd_remap());
      return launch_status(name);
    }
    if (L.kind == Kind::Narrow) {
      hipLaunchKernelGGL((sgemm_kernel<Plan, 2, 1, 0, true>), L.grid, dim3(THREADS), 0, st, pl, L.S,
                         static_cast<float*>(ws), xcd_remap());
      return reduce_splits(pl, L.S, static_cast<const float*>(ws), st, name);
    }
  }
  const int tile = 10 * L.ms + L.ns;
  if constexpr (wide_tiles<Plan>()) {
    switch (tile) {
      case 13: return launch_tiles<Plan, 1, 3>(pl, L, ws, ws_bytes, st, name);
      case 31: return launch_tiles<Plan, 3, 1>(pl, L, ws, ws_bytes, st, name);
      case 14: return launch_tiles<Plan, 1, 4>(pl, L, ws, ws_bytes, st, name);
      case 41: return launch_tiles<Plan, 4, 1>(pl, L, ws, ws_bytes, st, name);
      default: break;
    }
  }
  if constexpr (!std::is_base_of<BGemmArgs, Plan>::value) {  // the batched GEMMs: square tiles only
    if (tile == 21) return launch_tiles<Plan, 2, 1>(pl, L, ws, ws_bytes, st, name);
    if (tile == 12) return launch_tiles<Plan, 1, 2>(pl, L, ws, ws_bytes, st, name);
  }
  if (tile == 22) return launch_tiles<Plan, 2, 2>(pl, L, ws, ws_bytes, st, name);
  return launch_tiles<Plan, 1, 1>(pl, L, ws, ws_bytes, st, name);
}

inline bool shape_ok(int64_t Cin, int64_t Cout) { return Cin % 64 == 0 && Cout % 64 == 0; }

inline bool args_ok(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                    int64_t stride, int64_t pad) {
  if (!conv::geom_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad) || !shape_ok(Cin, Cout)) return false;
  // byte offsets inside one client's buffer view must fit the 31-bit voffset
  if (!(B * K * Cin * H * W * 4 < (int64_t(1) << 31) && B * K * Cout * H * W * 4 < (int64_t(1) << 31) &&
        KH * KW * Cin * Cout * 4 < (int64_t(1) << 31)))
    return false;
  // the kernels decode taps by rectangle arithmetic (true for any stride <= 4
  // conv whose live rows / columns are contiguous: every ResNet shape)
  if (stride > 4) return false;
  const conv::Geom g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  if (!g.rect.ok) return false;
  DgradT cls[MAX_CLASSES];
  const int nc = dgrad_classes(g, cls);
  for (int c = 0; c < nc; ++c)
    if (!cls[c].crect.ok) return false;
  return true;
}

}  // namespace convt
}  // namespace flr
