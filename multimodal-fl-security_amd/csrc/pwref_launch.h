// Reference-exact Krum distances: one host launcher per kernel family, defined
// beside its kernels (agg_pairwise_ref_{layout,dpp,quad}.hip), so the planner
// (agg_pairwise_ref.hip) needs no kernel definition.  Each enqueues on st and
// returns launch_status under its kernel's own name.
#pragma once
#include "pwref_common.h"

namespace flr {
namespace pwref {

// --- agg_pairwise_ref_layout.hip -------------------------------------------
// Xc[k][c][s] = X[k][8 (r0 + s) + c], the waves of `runs` (none: no launch)
int launch_chain_transpose(const float* X, int64_t K, int64_t ldx, int64_t r0, int64_t steps, int64_t ldc, float* Xc,
                           const WaveRuns& runs, hipStream_t st);
// block tb's coordinates inside chain steps [r0, r0 + steps), chain-major; the
// taps of mask `dead` read from gdead (negated on rows < nneg)
int launch_tap_chain(const float* X, int64_t K, int64_t ldx, const TapBlock& tb, int64_t r0, int64_t steps, int64_t ldc,
                     float* Xc, const float* gdead, uint64_t dead, int nneg, hipStream_t st);
// a dead region's compact form: the 3 x 3 block's live taps (plan `live`) at
// their slots of the live stream Xc
int launch_tap_chain_live(const float* X, int64_t K, int64_t ldx, const TapBlock& tb, int64_t r0, int64_t steps,
                          int64_t ldc, float* Xc, uint64_t dead, int nneg, const DeadPlan& live, hipStream_t st);
// slots [0, n0) and [z0, z1) of the 8 K streams zeroed
int launch_zero_slots(float* Xc, int64_t ldc, int64_t K, int n0, int64_t z0, int64_t z1, hipStream_t st);
// T = g + g at every dead coordinate's slot of block tb; *flag raised on a non-finite one
int launch_dead_stream(const float* g, const TapBlock& tb, const DeadPlan& deadp, int64_t ldt, float* T, int* flag,
                       hipStream_t st);
// Xq[c][b][k][e] = X[k][8 (r0 + 4 b + e) + c], NB blocks of Kp rows
int launch_quad_transpose(const float* X, int64_t ldx, int64_t K, int64_t r0, int64_t steps, int64_t NB, int64_t Kp,
                          float* Xq, hipStream_t st);

// --- agg_pairwise_ref_dpp.hip ------------------------------------------------
// tiles [t0, t1) over `steps` steps of Xc, continuing A (first: from 0)
int launch_ref_chain(const float* Xc, int64_t ldc, int64_t K, int64_t steps, int t0, int t1, int first, float* A,
                     hipStream_t st);
// every pair, two chains per lane
int launch_ref_chain2(const float* Xc, int64_t ldc, int64_t K, int64_t steps, int first, float* A, hipStream_t st);
// The dead-tap masks with a dead region form (ref_chain_dead_kernel<DM>): C3's
// one live tap (the centre) and its four (the 2 x 2 corner of a stride-2 block)
constexpr int DM_ONE = 0x1EF, DM_FOUR = 0x04F;
// every tile over a dead region's two streams, dm one of the masks above
int launch_ref_chain_dead(int dm, const float* Xl, int64_t ldc, const float* Tb, int64_t ldt, int64_t K, int nneg,
                          int64_t steps, int first, float* A, hipStream_t st);

// --- agg_pairwise_ref_quad.hip -----------------------------------------------
// the one-wave form, ni = 4 or 8 I rows per wave
int launch_ref_chain_s(int ni, const float* Xq, int64_t NB, int64_t Kp, int64_t K, int first, float* A, hipStream_t st);
// the workgroup form; xl: x_i through LDS (else scalar loads)
int launch_ref_chain_w(bool xl, const float* Xq, int64_t NB, int64_t Kp, int64_t K, int first, float* A,
                       hipStream_t st);

}  // namespace pwref
}  // namespace flr
