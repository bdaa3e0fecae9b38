// Internal helpers shared by the flr HIP translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>

#include "../../include/flr.h"

namespace flr {

// Records the last HIP error text for flr_last_error().
void set_last_error(const char* where, hipError_t e);

// An A/B switch's value (the FLR_* environment read once at library load, or
// flr_set_knob since), nullptr when unset (capi.cpp).
const char* knob(const char* name);
// The usual readings: "0..." turns a default-on path off, "1..." a default-off
// one on; an integer in [lo, hi], else (unset included) dflt.
inline bool knob_off(const char* name) {
  const char* e = knob(name);
  return e && e[0] == '0';
}
inline bool knob_on(const char* name) {
  const char* e = knob(name);
  return e && e[0] == '1';
}
inline int knob_int(const char* name, int lo, int hi, int dflt) {
  const char* e = knob(name);
  const int x = e ? atoi(e) : dflt;
  return e && x >= lo && x <= hi ? x : dflt;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Checks the launch that was just enqueued.
inline int launch_status(const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(where, e);
    return FLR_ERR_HIP;
  }
  return FLR_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// attack_colluding.hip: flr_collude_rows' launch.  mode STATS_ONLY writes no row
// of X, only mean_out / std_out — the same kernels, so the same bits
// (attack_minmax.hip's first stage).
namespace collude {
constexpr int STATS_ONLY = -1;
int launch(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal, int mode, float param, float* mean_out,
           float* std_out, hipStream_t st);
}  // namespace collude

__host__ __device__ constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// fp32 add/sub/mul/div with no contraction (the reference computes each op as a
// separate rounded torch op, so FMA contraction would break bit parity).
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }

// Correctly rounded fp32 sqrt (std::sqrt / torch's sqrt on the CPU).  HIP's
// __fsqrt_rn is the native v_sqrt_f32 (up to 1 ulp off) unless the OCML
// rounded operations are enabled, so the candidate is checked against the
// rounding midpoints in fp64 (exact: a midpoint has 25 significant bits, its
// square at most 50) and moved by one ulp when needed.
__device__ __forceinline__ float sqrt_rn(float s) {
  float r = __builtin_sqrtf(s);
  if (!(s > 0.f) || !(r < __builtin_huge_valf())) return r;  // 0, negative, NaN, inf
  const uint32_t u = __float_as_uint(r);
  const float up = __uint_as_float(u + 1), dn = __uint_as_float(u - 1);
  const double sd = (double)s, rd = (double)r;
  const double hi = 0.5 * (rd + (double)up);
  if (sd > hi * hi) return up;
  const double lo = 0.5 * (rd + (double)dn);
  if (sd < lo * lo) return dn;
  return r;
}

}  // namespace flr
