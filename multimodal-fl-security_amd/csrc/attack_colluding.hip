// a16 — the omniscient, colluding model-poisoning attacks on gfx950.
//
// ALIE (Baruch, Baruch, Goldberg, "A Little Is Enough", NeurIPS 2019): every
// attacker submits mu - z * sigma per coordinate; IPM (Xie, Koyejo, Gupta,
// "Fall of Empires", UAI 2019; the benign-mean branch of the reference's
// InnerProductManipulationAttack.poison_update, src/attacks/model_poisoning.py):
// every attacker submits -epsilon * mu.  mu and sigma are the mean and the
// population standard deviation of the benign rows [nmal, K) of the client
// matrix; the attackers' rows [0, nmal) are overwritten in place, all with the
// same vector.
//
// The arithmetic is fixed (flr.h): sequential fp32 adds over the benign rows in
// row order, every multiply and add rounded on its own, one correctly rounded
// division and square root — a torch CPU loop over the rows gives the same bits.
//
// Engine: one lane per coordinate, as agg_orderstat.hip — each load instruction
// reads 256 contiguous bytes of one row.  The pass is HBM-bound (it reads
// nb * P * 4 bytes and writes nmal * P * 4), and sigma needs the column twice
// (the mean, then the squared deviations): up to nb = 128 benign rows the lane
// keeps its column in VGPRs (template on the padded count), so the second pass
// costs no memory traffic.  Past that, and whenever sigma is not wanted at all
// (IPM with no std_out: a plain column sum), a streaming form walks the rows
// with 16 loads in flight (rows_pass.h's stream_rows) and, for sigma, walks them a second time — the same
// operations in the same order, so the same bits.
#include "rows_pass.h"

namespace flr {
namespace collude {

using rows::THREADS;
constexpr int GROUP = 8;  // rows per wave-uniform load group of the register form

template <int N>
__device__ __forceinline__ void reg_fence(float* v) {
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
}

// mu, sigma -> the attackers' rows and the optional outputs.  Every load of the
// column is done by now: the rows written here are never among the rows read.
// mode STATS_ONLY (attack_minmax.hip's first stage): the outputs alone.
__device__ __forceinline__ void finish(float* __restrict__ X, int64_t p, int64_t ldx, int64_t nmal, int mode,
                                       float param, float mu, float sigma, float* __restrict__ mean_out,
                                       float* __restrict__ std_out) {
  if (mode != STATS_ONLY) {  // wave-uniform
    const float a = mode == FLR_COLLUDE_ALIE ? sub_rn(mu, mul_rn(param, sigma)) : -mul_rn(param, mu);
    float* dst = X + p;
    for (int64_t r = 0; r < nmal; ++r) dst[r * ldx] = a;
  }
  if (mean_out) mean_out[p] = mu;
  if (std_out) std_out[p] = sigma;
}

// nb <= NP benign rows held in registers.  3 waves/SIMD as the order-statistic
// kernels: NP = 128 values and the few temporaries fit the 168 VGPRs.
template <int NP>
__global__ __launch_bounds__(THREADS, 3) void collude_reg_kernel(float* X, int nb, int64_t P, int64_t ldx,
                                                                   int64_t nmal, int mode, float param,
                                                                   float* mean_out, float* std_out) {
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (p >= P) return;
  const float* col = X + nmal * ldx + p;
  float v[NP];
  // Groups of GROUP rows behind one wave-uniform test each; inside a group the
  // row index is clamped instead of tested, so the loads issue back to back (a
  // padding register re-reads the last benign row and is never summed).
#pragma unroll
  for (int k0 = 0; k0 < NP; k0 += GROUP) {
    if (k0 < nb) {
#pragma unroll
      for (int k = k0; k < k0 + GROUP; ++k) v[k] = col[(int64_t)min(k, nb - 1) * ldx];
    } else {
#pragma unroll
      for (int k = k0; k < k0 + GROUP; ++k) v[k] = 0.f;
    }
  }
  // all NP values pinned in VGPRs between the phases (agg_orderstat.hip's note
  // on live ranges stretched across phases and the spills that follow)
  reg_fence<NP>(v);
  // whole groups behind one wave-uniform test (per-rank tests keep 2 SGPRs of
  // lane mask live per rank: 186 spilled at NP = 128); in the last, partial group
  // a padding rank adds +0.f: the sums start at +0.f and a round-to-nearest sum
  // is never -0.f from there, so that add is the identity (NaN included)
  float s = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < NP; k0 += GROUP) {
    if (k0 + GROUP <= nb) {
#pragma unroll
      for (int k = k0; k < k0 + GROUP; ++k) s = add_rn(s, v[k]);
    } else if (k0 < nb) {
#pragma unroll
      for (int k = k0; k < k0 + GROUP; ++k) s = add_rn(s, k < nb ? v[k] : 0.f);
    }
  }
  const float fnb = (float)nb;
  const float mu = div_rn(s, fnb);
  reg_fence<NP>(v);
  float q = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < NP; k0 += GROUP) {
    if (k0 + GROUP <= nb) {
#pragma unroll
      for (int k = k0; k < k0 + GROUP; ++k) {
        const float d = sub_rn(v[k], mu);
        q = add_rn(q, mul_rn(d, d));
      }
    } else if (k0 < nb) {
#pragma unroll
      for (int k = k0; k < k0 + GROUP; ++k) {
        const float d = sub_rn(v[k], mu);
        q = add_rn(q, k < nb ? mul_rn(d, d) : 0.f);
      }
    }
  }
  const float sigma = sqrt_rn(div_rn(q, fnb));
  finish(X, p, ldx, nmal, mode, param, mu, sigma, mean_out, std_out);
}

// Any nb: the rows streamed, STREAM loads in flight; SIGMA: streamed twice.
template <bool SIGMA>
__global__ __launch_bounds__(THREADS) void collude_stream_kernel(float* X, int64_t nb, int64_t P, int64_t ldx,
                                                                  int64_t nmal, int mode, float param,
                                                                  float* mean_out, float* std_out) {
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (p >= P) return;
  const float* col = X + nmal * ldx + p;
  const auto row = [](int64_t k) { return k; };
  float s = 0.f;
  rows::stream_rows<1>(col, ldx, nb, row, [&](int64_t, const float(&x)[1]) { s = add_rn(s, x[0]); });
  const float fnb = (float)nb;
  const float mu = div_rn(s, fnb);
  float sigma = 0.f;
  if constexpr (SIGMA) {
    float q = 0.f;
    rows::stream_rows<1>(col, ldx, nb, row, [&](int64_t, const float(&x)[1]) {
      const float d = sub_rn(x[0], mu);
      q = add_rn(q, mul_rn(d, d));
    });
    sigma = sqrt_rn(div_rn(q, fnb));
  }
  finish(X, p, ldx, nmal, mode, param, mu, sigma, mean_out, std_out);
}

int launch(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal, int mode, float param, float* mean_out,
           float* std_out, hipStream_t st) {
  const int64_t nblocks = (P + THREADS - 1) / THREADS;
  if (nblocks > 0x7fffffffLL) return FLR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)nblocks), block(THREADS);
  const int64_t nb = K - nmal;
  const bool sigma = mode == FLR_COLLUDE_ALIE || std_out != nullptr;
  if (!sigma)
    hipLaunchKernelGGL((collude_stream_kernel<false>), grid, block, 0, st, X, nb, P, ldx, nmal, mode, param,
                       mean_out, std_out);
  else if (nb <= 16)
    hipLaunchKernelGGL((collude_reg_kernel<16>), grid, block, 0, st, X, (int)nb, P, ldx, nmal, mode, param,
                       mean_out, std_out);
  else if (nb <= 32)
    hipLaunchKernelGGL((collude_reg_kernel<32>), grid, block, 0, st, X, (int)nb, P, ldx, nmal, mode, param,
                       mean_out, std_out);
  else if (nb <= 64)
    hipLaunchKernelGGL((collude_reg_kernel<64>), grid, block, 0, st, X, (int)nb, P, ldx, nmal, mode, param,
                       mean_out, std_out);
  else if (nb <= 128)
    hipLaunchKernelGGL((collude_reg_kernel<128>), grid, block, 0, st, X, (int)nb, P, ldx, nmal, mode, param,
                       mean_out, std_out);
  else
    hipLaunchKernelGGL((collude_stream_kernel<true>), grid, block, 0, st, X, nb, P, ldx, nmal, mode, param,
                       mean_out, std_out);
  return launch_status("collude_rows_kernel");
}

}  // namespace collude
}  // namespace flr

using namespace flr;

extern "C" int flr_collude_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal, int mode, float param,
                                float* mean_out, float* std_out, void* stream) {
  if (!X || K < 2 || nmal < 1 || nmal >= K || P < 1 || ldx < P ||
      (mode != FLR_COLLUDE_ALIE && mode != FLR_COLLUDE_IPM))
    return FLR_ERR_ARG;
  return collude::launch(X, K, P, ldx, nmal, mode, param, mean_out, std_out, as_stream(stream));
}
