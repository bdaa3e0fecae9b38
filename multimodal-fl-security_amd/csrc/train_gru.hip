// a3 — the text encoder's GRU recurrence (gate math) for all clients of a GPU.
//
// Reference layer: nn.GRU(embed, hidden, num_layers=1, batch_first=True), the
// second modality branch of the late-fusion model (BASELINE configs C2/C3;
// fusion structure src/models/cub200_cnn.py:88-117), trained per client in
// run_experiments.py:216-235.  torch's GRU cell (gate order r, z, n):
//   r = sigmoid(i_r + h_r)       z = sigmoid(i_z + h_z)
//   n = tanh(i_n + r * h_n)      h' = (h - n) * z + n
// with i = x W_ih^T + b_ih (whole sequence, one GEMM outside) and
// h_* = h W_hh^T + b_hh (one batched GEMM per step, outside).  These kernels
// are the per-step pointwise part: ONE launch per step forward and one per
// step backward replace torch's ~30 strided elementwise launches per step.
//
// Layouts (fp32, per GPU, K clients x B samples, hidden H, T steps):
//   gi    [K][B][T][3H]   input projections (the GEMM's natural output)
//   gh    [K][B][3H]      this step's hidden projections (bias included)
//   hseq  [K][T+1][B][H]  h_0 .. h_T (h_0 = 0), so hseq[k, 0:T] is the
//                         contiguous [T*B][H] operand of the dW_hh GEMM
//   gates [K][T][B][4][H] r, z, n, h_n saved for backward
//   dgh   [K][T][B][3H]   d(h W_hh^T + b_hh) per step, for dW_hh / db_hh
//   dgi   [K][B][T][3H]   d(gi)
#include "bf16x6.h"

#include <stdlib.h>
#include <string.h>

namespace flr {
namespace gru {

constexpr int THREADS = 256;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// One element's gate math from gi, gh = h W_hh^T + b_hh and h_t: every forward
// kernel calls this, so their r, z, n, h' agree bit for bit.
struct Gate {
  float r, z, n, h;
};
__device__ __forceinline__ Gate gate_math(float gir, float giz, float gin, float ghr, float ghz, float hn, float hp) {
  Gate o;
  o.r = sigm(gir + ghr);
  o.z = sigm(giz + ghz);
  o.n = tanhf(gin + o.r * hn);
  o.h = (hp - o.n) * o.z + o.n;  // h_{t+1}
  return o;
}

// One element's backward from dy = dL/dh_{t+1}: d(gh) = (drp, dzp, dnr),
// d(gi) = (drp, dzp, dnp), dhd = dL/dh_t through the z-gate path.  Every
// backward kernel calls this.
struct ElemBwd {
  float drp, dzp, dnp, dnr, dhd;
};
__device__ __forceinline__ ElemBwd elem_bwd(float dy, float r, float z, float n, float hn, float hp) {
  const float dz = dy * (hp - n);
  const float dn = dy * (1.0f - z);
  const float dnp = dn * (1.0f - n * n);
  const float dr = dnp * hn;
  ElemBwd o;
  o.drp = dr * (r * (1.0f - r));
  o.dzp = dz * (z * (1.0f - z));
  o.dnp = dnp;
  o.dnr = dnp * r;
  o.dhd = dy * z;
  return o;
}

struct Dims {
  int K, B, T, H, t;
  int wshared;  // 1: every client reads the one packed W_hh copy (the first local step)
};

__device__ __forceinline__ void decompose(const Dims& d, int64_t idx, int& k, int& b, int& j) {
  j = (int)(idx % d.H);
  const int64_t kb = idx / d.H;
  b = (int)(kb % d.B);
  k = (int)(kb / d.B);
}

__global__ __launch_bounds__(THREADS) void fwd_step_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                           float* __restrict__ hseq, float* __restrict__ gates,
                                                           const Dims d) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)d.K * d.B * d.H) return;
  int k, b, j;
  decompose(d, idx, k, b, j);
  const int H = d.H;
  const int64_t kb = (int64_t)k * d.B + b;
  const float* gir = gi + (kb * d.T + d.t) * 3 * H;
  const float* ghr = gh + kb * 3 * H;
  const int64_t hrow = (((int64_t)k * (d.T + 1) + d.t) * d.B + b) * H;
  const float hp = hseq[hrow + j];
  const float hn = ghr[2 * H + j];
  const Gate o = gate_math(gir[j], gir[H + j], gir[2 * H + j], ghr[j], ghr[H + j], hn, hp);
  hseq[hrow + (int64_t)d.B * H + j] = o.h;
  float* g = gates + (((int64_t)k * d.T + d.t) * d.B + b) * 4 * H;
  g[j] = o.r;
  g[H + j] = o.z;
  g[2 * H + j] = o.n;
  g[3 * H + j] = hn;
}

// dh: dL/dh_{t+1} [K][B][H]; writes dgh[:, t], dgi[:, :, t] and
// dh_direct = dL/dh_t through the z-gate path (the W_hh path is the caller's GEMM).
__global__ __launch_bounds__(THREADS) void bwd_step_kernel(const float* __restrict__ dh,
                                                           const float* __restrict__ gates,
                                                           const float* __restrict__ hseq, float* __restrict__ dgh,
                                                           float* __restrict__ dgi, float* __restrict__ dh_direct,
                                                           const Dims d) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)d.K * d.B * d.H) return;
  int k, b, j;
  decompose(d, idx, k, b, j);
  const int H = d.H;
  const int64_t kb = (int64_t)k * d.B + b;
  const int64_t srow = ((int64_t)k * d.T + d.t) * d.B + b;
  const float* g = gates + srow * 4 * H;
  const float r = g[j], z = g[H + j], n = g[2 * H + j], hn = g[3 * H + j];
  const float hp = hseq[(((int64_t)k * (d.T + 1) + d.t) * d.B + b) * H + j];
  const ElemBwd eb = elem_bwd(dh[idx], r, z, n, hn, hp);
  float* o = dgh + srow * 3 * H;
  o[j] = eb.drp;
  o[H + j] = eb.dzp;
  o[2 * H + j] = eb.dnr;
  float* q = dgi + (kb * d.T + d.t) * 3 * H;
  q[j] = eb.drp;
  q[H + j] = eb.dzp;
  q[2 * H + j] = eb.dnp;
  dh_direct[idx] = eb.dhd;
}

// ---- fused per-step kernels: the recurrence GEMM with the gate math in its
// epilogue.  One wave per (client, 32 hidden units); B <= 32 batch rows are the
// MFMA's 32 rows.  fp32 operands split into three bf16 terms, six products per
// 16-deep k-step on v_mfma_f32_32x32x16_bf16 (the bf16x6 form of the batched
// GEMM: per-product error a few 2^-24 |a b|).  The forward reads W_hh rows
// ([3H][H], k-contiguous); the backward reads W_hh^T ([H][3H], transposed once
// per optimizer step by flr_gru_transpose) so both operands load k-contiguous.
// The split (split3_sub), the product order (mfma6) and the raw buffer loads are
// bf16x6.h's: an out-of-range byte offset returns 0 with no branch, so a wave's
// loads of several k-steps stay in flight together (a per-lane branch would join
// through register moves that wait on each load).

// 8 floats of a row starting at k0; zeros for an invalid row or past R.  V8: R
// and k0 are multiples of 8, so k0 < R covers all 8.
template <bool V8>
__device__ __forceinline__ void bload8(rsrc_t r, bool ok, int row_off, int k0, int R, float (&v)[8]) {
  if constexpr (V8) {
    const unsigned off = (ok && k0 < R) ? (unsigned)(row_off + k0) * 4u : SENT;
    const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    const f32x4 y = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off + 16u, 0, 0));
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned off = (ok && k0 + e < R) ? (unsigned)(row_off + k0 + e) * 4u : SENT;
      v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
    }
  }
}

// Packed weights (flr_gru_pack): for a 32-row block `blk` and k-step s, the 64
// lanes' 8-float B fragments as two contiguous 1 KB halves,
//   wp[((blk * S + s) * 2 + q) * 256 + lane * 4 + e] = W[blk row (lane & 31)][16 s + 8 (lane >> 5) + 4 q + e]
// zero-padded, so one b128 per half reads 1 KB contiguous across the wave.
__device__ __forceinline__ void pload8(rsrc_t r, bool in, int blk, int S, int s, int lane, float (&v)[8]) {
  const unsigned off = in ? (unsigned)(((blk * S + s) * 2) * 256 + lane * 4) * 4u : SENT;
  const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
  const f32x4 y = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off + 1024u, 0, 0));
  v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
  v[4] = y[0]; v[5] = y[1]; v[6] = y[2]; v[7] = y[3];
}

// Workgroup -> (client, 32-unit block).  Workgroups go round-robin over the 8
// XCDs by linear id; remap so one client's unit blocks share an XCD (and its L2:
// they all read the same h_t / dgh_t rows).
__device__ __forceinline__ void block_coords(int nub, int& k, int& ub) {
  const int n = gridDim.x, L = blockIdx.x;
  const int idx = (n % 8 == 0) ? (L % 8) * (n / 8) + L / 8 : L;
  k = idx / nub;
  ub = idx % nub;
}

// The k-steps (16 deep) are split over the NW waves of a workgroup in contiguous
// ranges; each wave issues the loads of G k-steps before their MFMAs, and the
// NW partial accumulators are summed in wave order through LDS (deterministic).
// Every loop bound is wave-uniform: the MFMA needs all 64 lanes.  The epilogue's
// operands (16 x 64 elements over the workgroup) are loaded before the GEMM.
__device__ __forceinline__ float bload1(rsrc_t r, bool ok, int64_t off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, ok ? (unsigned)off * 4u : SENT, 0, 0));
}

// forward step t: gh = h_t W_hh^T + b_hh for the units [j0, j0+32) of all three
// gates, then the gate math of fwd_step_kernel for those units.
// SEQ: the waves' partial sums added in wave order through ONE LDS slot (wave w
// adds its partials to the slot in turn: the same sums in the same order as
// the NW-slot form, bit-identical), 12 KB instead of 96 KB of LDS, and the
// kernel held to 128 VGPRs, so two workgroups share a CU and one's W_hh
// stream overlaps the other's reduction and gate math (the NW-slot form runs
// one workgroup per CU: 1024 workgroups in four serial rounds at C3).
template <bool V8, int NW, int G, bool SEQ = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(SEQ ? 4 : 1))) void fwd_fused_kernel(const float* __restrict__ gi,
                                                            const float* __restrict__ whhP,
                                                            const float* __restrict__ bhh, float* __restrict__ hseq,
                                                            float* __restrict__ gates, const Dims d, int nub) {
  constexpr int EPT = 16 / NW;  // epilogue elements per thread
  __shared__ float red[SEQ ? 1 : NW][3][16][64];
  int k, ub;
  block_coords(nub, k, ub);
  const int j0 = ub * 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
  const int B = d.B, H = d.H;
  const rsrc_t rh = make_rsrc(hseq + ((int64_t)k * (d.T + 1) + d.t) * B * H, (int64_t)B * H);
  const int S = (H + 15) / 16, per = (S + NW - 1) / NW;
  const rsrc_t rw = make_rsrc(whhP + (d.wshared ? 0 : (int64_t)k * 3 * nub * S * 512), (int64_t)3 * nub * S * 512);
  const rsrc_t rg = make_rsrc(gi + (int64_t)k * B * d.T * 3 * H, (int64_t)B * d.T * 3 * H);
  const rsrc_t rbias = make_rsrc(bhh + (int64_t)k * 3 * H, (int64_t)3 * H);
  // epilogue operands: element p = tid + 64 NW i -> (e, ln) of the MFMA tile
  float pgi[EPT][3], php[EPT], pbh[EPT][3];
  auto load_epi = [&]() {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int p = threadIdx.x + 64 * NW * i, e = p >> 6, ln = p & 63;
      const int b = (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5), j = j0 + (ln & 31);
      const bool ok = b < B && j < H;
      const int64_t go = ((int64_t)b * d.T + d.t) * 3 * H + j;
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        pgi[i][g] = bload1(rg, ok, go + g * H);
        pbh[i][g] = bload1(rbias, ok, g * H + j);
      }
      php[i] = bload1(rh, ok, (int64_t)b * H + j);
    }
  };
  // SEQ: the epilogue operands are loaded after the MFMAs (their latency under the
  // ordered reduction), keeping them out of the loads' register peak
  if constexpr (!SEQ) load_epi();
  const bool aok = l32 < B;
  f32x16 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;
  const int s1 = min(S, (wave + 1) * per);
  for (int s = wave * per; s < s1; s += G) {
    float a[G][8], b[G][3][8];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      const bool in = s + q < s1;
      const int k0 = (s + q) * 16 + 8 * h;
      bload8<V8>(rh, aok && in, l32 * H, k0, H, a[q]);
#pragma unroll
      for (int g = 0; g < 3; ++g) pload8(rw, in, g * nub + ub, S, s + q, lane, b[q][g]);
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of the group issued before the first MFMA
#pragma unroll
    for (int q = 0; q < G; ++q) {
      bf16x8 ah, am, al;
      split3_sub(a[q], ah, am, al);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        bf16x8 bh, bm, bl;
        split3_sub(b[q][g], bh, bm, bl);
        acc[g] = mfma6(acc[g], ah, am, al, bh, bm, bl);
      }
    }
  }
  if constexpr (SEQ) {
    load_epi();
    for (int w = 0; w < NW; ++w) {
      if (wave == w)
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int e = 0; e < 16; ++e) red[0][g][e][lane] = w == 0 ? acc[g][e] : red[0][g][e][lane] + acc[g][e];
      __syncthreads();
    }
  } else {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 16; ++e) red[wave][g][e][lane] = acc[g][e];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int p = threadIdx.x + 64 * NW * i, e = p >> 6, ln = p & 63;
    const int b = (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5), j = j0 + (ln & 31);
    if (b >= B || j >= H) continue;
    float v[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      float x = red[0][g][e][ln];
      if constexpr (!SEQ)
#pragma unroll
        for (int w = 1; w < NW; ++w) x += red[w][g][e][ln];
      v[g] = x;
    }
    const int64_t hrw = (((int64_t)k * (d.T + 1) + d.t) * B + b) * H;
    const float ghr = pbh[i][0] + v[0], ghz = pbh[i][1] + v[1], hn = pbh[i][2] + v[2];
    const Gate o = gate_math(pgi[i][0], pgi[i][1], pgi[i][2], ghr, ghz, hn, php[i]);
    hseq[hrw + (int64_t)B * H + j] = o.h;
    float* gg = gates + (((int64_t)k * d.T + d.t) * B + b) * 4 * H;
    gg[j] = o.r;
    gg[H + j] = o.z;
    gg[2 * H + j] = o.n;
    gg[3 * H + j] = hn;
  }
}

// backward step t >= 1: dh_t = dh_direct + dgh_t W_hh for the units [i0, i0+32)
// (W_hh^T rows), then the element backward of step t - 1 for those units
// (d.t = t - 1).  dh_direct is read and rewritten in place by the same thread.
template <bool V8, int NW, int G, bool SEQ = false>  // SEQ: as fwd_fused_kernel's
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(SEQ ? 6 : 1))) void bwd_fused_kernel(const float* __restrict__ whhTP,
                                                            const float* __restrict__ gates,
                                                            const float* __restrict__ hseq, float* __restrict__ dgh,
                                                            float* __restrict__ dgi, float* __restrict__ dh_direct,
                                                            float* __restrict__ dh0, const Dims d, int nub) {
  constexpr int EPT = 16 / NW;
  __shared__ float red[SEQ ? 1 : NW][16][64];
  int k, ub;
  block_coords(nub, k, ub);
  const int i0 = ub * 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
  const int B = d.B, H = d.H, R = 3 * H;
  const int t = d.t + 1;  // this launch's GEMM step
  const rsrc_t ra = make_rsrc(dgh + ((int64_t)k * d.T + t) * B * R, (int64_t)B * R);
  const int S = (R + 15) / 16, per = (S + NW - 1) / NW;
  const rsrc_t rb = make_rsrc(whhTP + (d.wshared ? 0 : (int64_t)k * nub * S * 512), (int64_t)nub * S * 512);
  const rsrc_t rdd = make_rsrc(dh_direct + (int64_t)k * B * H, (int64_t)B * H);
  // epilogue operands: dh_direct, and step t-1's gates and h_{t-1} when d.t >= 0
  const bool elem = d.t >= 0;
  const int tg = elem ? d.t : 0;
  const rsrc_t rgt = make_rsrc(gates + ((int64_t)k * d.T + tg) * B * 4 * H, (int64_t)B * 4 * H);
  const rsrc_t rhp = make_rsrc(hseq + ((int64_t)k * (d.T + 1) + tg) * B * H, (int64_t)B * H);
  float pdd[EPT], pg[EPT][4], php[EPT];
  auto load_epi = [&]() {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int p = threadIdx.x + 64 * NW * i, e = p >> 6, ln = p & 63;
      const int b = (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5), j = i0 + (ln & 31);
      const bool ok = b < B && j < H;
      pdd[i] = bload1(rdd, ok, (int64_t)b * H + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) pg[i][q] = bload1(rgt, ok && elem, (int64_t)b * 4 * H + q * H + j);
      php[i] = bload1(rhp, ok && elem, (int64_t)b * H + j);
    }
  };
  if constexpr (!SEQ) load_epi();
  const bool aok = l32 < B;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int s1 = min(S, (wave + 1) * per);
  for (int s = wave * per; s < s1; s += G) {
    float a[G][8], b[G][8];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      const bool in = s + q < s1;
      const int k0 = (s + q) * 16 + 8 * h;
      bload8<V8>(ra, aok && in, l32 * R, k0, R, a[q]);
      pload8(rb, in, ub, S, s + q, lane, b[q]);
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of the group issued before the first MFMA
#pragma unroll
    for (int q = 0; q < G; ++q) {
      bf16x8 ah, am, al, bh, bm, bl;
      split3_sub(a[q], ah, am, al);
      split3_sub(b[q], bh, bm, bl);
      acc = mfma6(acc, ah, am, al, bh, bm, bl);
    }
  }
  if constexpr (SEQ) {
    load_epi();
    for (int w = 0; w < NW; ++w) {
      if (wave == w)
#pragma unroll
        for (int e = 0; e < 16; ++e) red[0][e][lane] = w == 0 ? acc[e] : red[0][e][lane] + acc[e];
      __syncthreads();
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave][e][lane] = acc[e];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int p = threadIdx.x + 64 * NW * i, e = p >> 6, ln = p & 63;
    const int b = (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5), j = i0 + (ln & 31);
    if (b >= B || j >= H) continue;
    float x = red[0][e][ln];
    if constexpr (!SEQ)
#pragma unroll
      for (int w = 1; w < NW; ++w) x += red[w][e][ln];
    const int64_t kb = (int64_t)k * B + b;
    const int64_t idx = kb * H + j;
    const float dy = pdd[i] + x;  // dL/dh_t
    if (dh0) dh0[idx] = dy;
    if (!elem) continue;
    // step t-1's element backward (bwd_step_kernel's math)
    const ElemBwd eb = elem_bwd(dy, pg[i][0], pg[i][1], pg[i][2], pg[i][3], php[i]);
    const int64_t srow = ((int64_t)k * d.T + d.t) * B + b;
    float* o = dgh + srow * 3 * H;
    o[j] = eb.drp;
    o[H + j] = eb.dzp;
    o[2 * H + j] = eb.dnr;
    float* q = dgi + (kb * d.T + d.t) * 3 * H;
    q[j] = eb.drp;
    q[H + j] = eb.dzp;
    q[2 * H + j] = eb.dnp;
    dh_direct[idx] = eb.dhd;
  }
}

// Pack a client's weight into the fused kernels' fragment order (pload8).  The
// packed operand is the [NG * H][C] matrix of rows (g, r) and columns c with
//   TRANS = 0: element = w[(g H + r) C + c]   (W_hh, [3H][H]: NG = 3, C = H)
//   TRANS = 1: element = w[c H + r]           (W_hh^T of a [C][H] W_hh: NG = 1, C = 3H)
// Row blocks of 32 per group (the last one zero-padded), k-steps of 16 (padded).
// One workgroup per (client, row block, 128-column chunk) through an LDS tile.
template <int TRANS>
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ w, int NG, int H, int C,
                                                   float* __restrict__ wp) {
  __shared__ float tile[32][129];
  const int k = blockIdx.z, blk = blockIdx.y, c0 = blockIdx.x * 128;
  const int nub = (H + 31) / 32, S = (C + 15) / 16;
  const int g = blk / nub, r0 = (blk % nub) * 32;
  const float* src = w + (int64_t)k * NG * H * C;
  for (int e = threadIdx.x; e < 32 * 128; e += 256) {
    int r, c;
    if (TRANS) { c = e >> 5; r = e & 31; } else { r = e >> 7; c = e & 127; }
    const bool ok = r0 + r < H && c0 + c < C;
    const int64_t off = TRANS ? (int64_t)(c0 + c) * H + r0 + r : ((int64_t)g * H + r0 + r) * C + c0 + c;
    tile[r][c] = ok ? src[off] : 0.f;
  }
  __syncthreads();
  float* dst = wp + ((int64_t)k * NG * nub + blk) * S * 512;
  for (int o = threadIdx.x; o < 8 * 512; o += 256) {  // the 8 k-steps of this chunk
    const int sl = o >> 9, q = (o >> 8) & 1, lane = (o >> 2) & 63, e = o & 3;
    const int s = c0 / 16 + sl;
    if (s < S) dst[(int64_t)s * 512 + q * 256 + lane * 4 + e] = tile[lane & 31][sl * 16 + 8 * (lane >> 5) + 4 * q + e];
  }
}

// ---- the whole recurrence in one launch per pass.  One workgroup per client
// loops over the time steps itself; wave ub owns the unit block ub that a
// per-step workgroup (k, ub) owns, so no workgroup ever waits on another and
// __syncthreads is the only synchronisation.  H % 32 == 0, H <= SEQ_HMAX; H is
// a template parameter, so every k-step's weight offset is a constant and the
// k-steps a range does not have are not compiled at all.
//
// Bit identity with the per-step default form ("8,2"): there an output
// element's GEMM sum is SEQ_NW partials, partial w accumulated from zero over
// wave w's k-steps [w per, min(S, (w + 1) per)) in order, then added
// x = p0; x += p1; ...  Here the one wave computes the same partials over the
// same ranges and adds them in the same order in registers.  (A partial is
// never -0: its accumulator starts at +0, so the per-step form's MFMAs on the
// zero operands of an idle k-step change nothing and are not issued here.)
//
// The A operand (h_t forward, dgh_t backward) is split once per step into its
// three bf16 term images in LDS, rows padded by 16 bytes (a row of 2 H bytes
// would put all 32 rows on the same banks); rows >= B stay zero, the zeros the
// per-step loads return.  The packed-weight loads of range w + 1 — and across
// the step boundary those of range 0, which do not depend on h — are issued
// before range w's MFMAs.
constexpr int SEQ_NW = 8;
constexpr int SEQ_HMAX = 256;

// tile row of accumulator register e for lane half h (mfma_f32_32x32x16's C map)
__device__ __forceinline__ int tile_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// GEMM geometry of a pass: NG row groups of NUB 32-row blocks, S k-steps
template <int NG_, int NUB_, int S_>
struct SeqGeo {
  static constexpr int NG = NG_, NUB = NUB_, S = S_;
  static constexpr int PER = (S + SEQ_NW - 1) / SEQ_NW;  // the per-step form's k-steps per wave
  static constexpr int RS = 16 * S + 8;                  // image row stride (bf16)
  static constexpr int IMG = 96 * RS;                    // three 32-row term images
};
template <class G>
using WBuf = float[G::PER][G::NG][8];

// The packed B fragments of range W: rw is based at this wave's block of group
// 0, voff = lane * 16; the (group, k-step) offset rides in the scalar offset.
template <class G, int W>
__device__ __forceinline__ void wload(rsrc_t rw, unsigned voff, WBuf<G>& v) {
#pragma unroll
  for (int q = 0; q < G::PER; ++q) {
    const int s = W * G::PER + q;
    if (s < G::S) {
#pragma unroll
      for (int g = 0; g < G::NG; ++g) {
        const int soff = ((g * G::NUB * G::S + s) * 512) * 4;
        const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, voff, soff, 0));
        const f32x4 y = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, voff, soff + 1024, 0));
        v[q][g][0] = x[0]; v[q][g][1] = x[1]; v[q][g][2] = x[2]; v[q][g][3] = x[3];
        v[q][g][4] = y[0]; v[q][g][5] = y[1]; v[q][g][6] = y[2]; v[q][g][7] = y[3];
      }
    }
  }
}

// partial W from zero over its k-steps, A fragments from the term images
// (a: this lane's row and k half of the first image), then x = p or x += p
template <class G, int W>
__device__ __forceinline__ void wmma(const __bf16* a, const WBuf<G>& v, f32x16 (&x)[G::NG]) {
  f32x16 p[G::NG];
#pragma unroll
  for (int g = 0; g < G::NG; ++g)
#pragma unroll
    for (int e = 0; e < 16; ++e) p[g][e] = 0.f;
#pragma unroll
  for (int q = 0; q < G::PER; ++q) {
    const int s = W * G::PER + q;
    if (s < G::S) {
      const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a + 16 * s);
      const bf16x8 am = *reinterpret_cast<const bf16x8*>(a + 16 * s + 32 * G::RS);
      const bf16x8 al = *reinterpret_cast<const bf16x8*>(a + 16 * s + 64 * G::RS);
#pragma unroll
      for (int g = 0; g < G::NG; ++g) {
        bf16x8 bh, bm, bl;
        split3_sub(v[q][g], bh, bm, bl);
        p[g] = mfma6(p[g], ah, am, al, bh, bm, bl);
      }
      __builtin_amdgcn_sched_barrier(0);  // one k-step's fragments live at a time: the register budget is 256
    }
  }
#pragma unroll
  for (int g = 0; g < G::NG; ++g)
#pragma unroll
    for (int e = 0; e < 16; ++e) x[g][e] = W == 0 ? p[g][e] : x[g][e] + p[g][e];
  // the sum is formed here: left free, the compiler keeps all SEQ_NW partials
  // alive and sinks these adds into the epilogue's per-row branches
#pragma unroll
  for (int g = 0; g < G::NG; ++g) asm volatile("" : "+v"(x[g]));
}

// One fp32 value into the three term images: p is the lane's part of the
// address (its 4 h rows and its column), off the element's constant part.
template <class G>
__device__ __forceinline__ void img_put(__bf16* p, int off, float v) {
  __bf16 a, b, c;
  split1_sub(v, a, b, c);
  p[off] = a;
  p[off + 32 * G::RS] = b;
  p[off + 64 * G::RS] = c;
}

// The SEQ_NW ranges of one GEMM, two register buffers alternating: range W + 1
// loads under range W's MFMAs; `last` (the epilogue's operand loads) is issued
// under the last range's.  On entry bA holds range 0; on exit it is free.
template <class G, int W = 0, class Last>
__device__ __forceinline__ void wgemm(const __bf16* a, rsrc_t rw, unsigned voff, WBuf<G>& bA, WBuf<G>& bB,
                                      f32x16 (&x)[G::NG], Last last) {
  wload<G, W + 1>(rw, voff, bB);
  __builtin_amdgcn_sched_barrier(0);
  wmma<G, W>(a, bA, x);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (W + 2 < SEQ_NW)
    wload<G, W + 2>(rw, voff, bA);
  else
    last();
  __builtin_amdgcn_sched_barrier(0);
  wmma<G, W + 1>(a, bB, x);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (W + 2 < SEQ_NW) wgemm<G, W + 2>(a, rw, voff, bA, bB, x, last);
}

// Epilogue element e of a lane is tile row tile_row(e, 0) + 4 h: its address in
// any of the arrays is one per-lane byte offset (the 4 h rows and the column)
// plus a wave-uniform one (the row's e part, the time step), which rides in the
// scalar offset, so an array costs one address register, not one per element.
__device__ __forceinline__ float ldg(rsrc_t r, unsigned voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void stg(rsrc_t r, float v, unsigned voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
}
// keeps the per-element offsets derived from v out of the registers across the time loop
__device__ __forceinline__ unsigned per_step(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int H>
__global__ __launch_bounds__(2 * H) void fwd_seq_kernel(const float* __restrict__ gi, const float* __restrict__ whhP,
                                                        const float* __restrict__ bhh, float* __restrict__ hseq,
                                                        float* __restrict__ gates, const Dims d) {
  using G = SeqGeo<3, H / 32, H / 16>;
  __shared__ __attribute__((aligned(16))) __bf16 img[2 * G::IMG];  // two h images: one barrier per step
  const int k = blockIdx.x, ub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int l32 = lane & 31, h = lane >> 5, j = ub * 32 + l32;
  const int B = d.B, T = d.T;
  for (int i = threadIdx.x * 8; i < 2 * G::IMG; i += 2 * H * 8)
    *reinterpret_cast<f32x4*>(img + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  constexpr int64_t WN = (int64_t)3 * G::NUB * G::S * 512;  // a client's packed floats
  const rsrc_t rw = make_rsrc(whhP + (d.wshared ? 0 : k * WN) + ub * G::S * 512, WN - ub * G::S * 512);
  const rsrc_t rg = make_rsrc(gi + (int64_t)k * B * T * 3 * H, (int64_t)B * T * 3 * H);
  const rsrc_t rbias = make_rsrc(bhh + (int64_t)k * 3 * H, (int64_t)3 * H);
  const rsrc_t rh = make_rsrc(hseq + (int64_t)k * (T + 1) * B * H, (int64_t)(T + 1) * B * H);
  const rsrc_t rgt = make_rsrc(gates + (int64_t)k * T * B * 4 * H, (int64_t)T * B * 4 * H);
  const unsigned voff = lane * 16;
  const unsigned vgi = (4 * h * T * 3 * H + j) * 4, vh = (4 * h * H + j) * 4, vgt = (4 * h * 4 * H + j) * 4;
  WBuf<G> bA, bB;
  wload<G, 0>(rw, voff, bA);
  float hp[16], pbh[3];  // this lane's h_t (the value it stored as h_{t+1} a step earlier) and bias
#pragma unroll
  for (int g = 0; g < 3; ++g) pbh[g] = bload1(rbias, true, g * H + j);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int b = tile_row(e, h);
    hp[e] = ldg(rh, b < B ? vh : SENT, tile_row(e, 0) * H * 4);
    if (b < B) img_put<G>(img + 4 * h * G::RS + j, tile_row(e, 0) * G::RS, hp[e]);
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const __bf16* cur = img + (t & 1) * G::IMG + l32 * G::RS + 8 * h;
    __bf16* nxt = img + ((t + 1) & 1) * G::IMG + 4 * h * G::RS + j;
    f32x16 x[3];
    float pgi[16][3];
    wgemm<G>(cur, rw, voff, bA, bB, x, [&]() {
      const unsigned v = per_step(vgi);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned off = tile_row(e, h) < B ? v : SENT;
#pragma unroll
        for (int g = 0; g < 3; ++g) pgi[e][g] = ldg(rg, off + g * H * 4, ((tile_row(e, 0) * T + t) * 3 * H) * 4);
      }
    });
    wload<G, 0>(rw, voff, bA);  // the next step's first range under the gate math (unused after the last step)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int b = tile_row(e, h);
      if (b < B) {
        const float ghr = pbh[0] + x[0][e], ghz = pbh[1] + x[1][e], hn = pbh[2] + x[2][e];
        const Gate o = gate_math(pgi[e][0], pgi[e][1], pgi[e][2], ghr, ghz, hn, hp[e]);
        stg(rh, o.h, vh, (((t + 1) * B + tile_row(e, 0)) * H) * 4);
        const int sg = ((t * B + tile_row(e, 0)) * 4 * H) * 4;
        stg(rgt, o.r, vgt, sg);
        stg(rgt, o.z, vgt + H * 4, sg);
        stg(rgt, o.n, vgt + 2 * H * 4, sg);
        stg(rgt, hn, vgt + 3 * H * 4, sg);
        hp[e] = o.h;
        img_put<G>(nxt, tile_row(e, 0) * G::RS, o.h);
      }
      __builtin_amdgcn_sched_barrier(0);  // one element's exp / tanh temporaries at a time
    }
    __syncthreads();  // h_{t+1}'s image complete; every wave is done reading h_t's (rewritten a step later)
  }
}

// dh: dL/dh_T [K][B][H].  Phase 1 is bwd_step_kernel at T-1; then the fused
// steps t = T-1 .. 1.  dgh_t reaches the next GEMM through its term images in
// LDS (one buffer of 3 x 32 x (3H + 8) bf16: 146 KB at H = 256, so two barriers
// per step) and is stored to HBM for the dW_hh GEMM as the per-step path does.
// dh_direct stays in registers between steps; the last step's is stored.
template <int H>
__global__ __launch_bounds__(2 * H) void bwd_seq_kernel(const float* __restrict__ whhTP,
                                                        const float* __restrict__ gates,
                                                        const float* __restrict__ hseq, const float* __restrict__ dh,
                                                        float* __restrict__ dgh, float* __restrict__ dgi,
                                                        float* __restrict__ dh_direct, float* __restrict__ dh0,
                                                        const Dims d) {
  using G = SeqGeo<1, H / 32, 3 * H / 16>;
  constexpr int R = 3 * H;
  __shared__ __attribute__((aligned(16))) __bf16 img[G::IMG];
  const int k = blockIdx.x, ub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int l32 = lane & 31, h = lane >> 5, j = ub * 32 + l32;
  const int B = d.B, T = d.T;
  for (int i = threadIdx.x * 8; i < G::IMG; i += 2 * H * 8)
    *reinterpret_cast<f32x4*>(img + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  constexpr int64_t WN = (int64_t)G::NUB * G::S * 512;
  const rsrc_t rw = make_rsrc(whhTP + (d.wshared ? 0 : k * WN) + ub * G::S * 512, WN - ub * G::S * 512);
  const rsrc_t rgt = make_rsrc(gates + (int64_t)k * T * B * 4 * H, (int64_t)T * B * 4 * H);
  const rsrc_t rhp = make_rsrc(hseq + (int64_t)k * (T + 1) * B * H, (int64_t)(T + 1) * B * H);
  const rsrc_t rdgh = make_rsrc(dgh + (int64_t)k * T * B * R, (int64_t)T * B * R);
  const rsrc_t rdgi = make_rsrc(dgi + (int64_t)k * B * T * R, (int64_t)B * T * R);
  const rsrc_t rdd = make_rsrc(dh_direct + (int64_t)k * B * H, (int64_t)B * H);
  const rsrc_t rdh0 = make_rsrc(dh0 ? dh0 + (int64_t)k * B * H : nullptr, dh0 ? (int64_t)B * H : 0);
  const unsigned vh = (4 * h * H + j) * 4, vgt = (4 * h * 4 * H + j) * 4, vgh = (4 * h * R + j) * 4;
  const unsigned vgi = (4 * h * T * R + j) * 4;
  float pg[16][4], php[16];  // the gates and h_t of the element step about to run
  auto load_epi = [&](int t) {
    const unsigned v4 = per_step(vgt), v1 = per_step(vh);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool ok = tile_row(e, h) < B;
      const int rowt = t * B + tile_row(e, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) pg[e][q] = ldg(rgt, (ok ? v4 : SENT) + q * H * 4, rowt * 4 * H * 4);
      php[e] = ldg(rhp, ok ? v1 : SENT, rowt * H * 4);
    }
  };
  float dd[16];  // dh_direct of this lane's elements
  // the element backward of step t from dy, its stores, and dgh_t's image (rows b < B only)
  auto elem = [&](int t, int e, float dy) {
    const ElemBwd eb = elem_bwd(dy, pg[e][0], pg[e][1], pg[e][2], pg[e][3], php[e]);
    const int so = ((t * B + tile_row(e, 0)) * R) * 4, si = ((tile_row(e, 0) * T + t) * R) * 4;
    stg(rdgh, eb.drp, vgh, so);
    stg(rdgh, eb.dzp, vgh + H * 4, so);
    stg(rdgh, eb.dnr, vgh + 2 * H * 4, so);
    stg(rdgi, eb.drp, vgi, si);
    stg(rdgi, eb.dzp, vgi + H * 4, si);
    stg(rdgi, eb.dnp, vgi + 2 * H * 4, si);
    dd[e] = eb.dhd;
    if (t == 0) {
      stg(rdd, eb.dhd, vh, tile_row(e, 0) * H * 4);
    } else {
      __bf16* p = img + 4 * h * G::RS + j;
      img_put<G>(p, tile_row(e, 0) * G::RS, eb.drp);
      img_put<G>(p, tile_row(e, 0) * G::RS + H, eb.dzp);
      img_put<G>(p, tile_row(e, 0) * G::RS + 2 * H, eb.dnr);
    }
  };
  load_epi(T - 1);
  {
    const rsrc_t rdh = make_rsrc(dh + (int64_t)k * B * H, (int64_t)B * H);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const bool ok = tile_row(e, h) < B;
      const float dy = ldg(rdh, ok ? vh : SENT, tile_row(e, 0) * H * 4);
      if (ok) elem(T - 1, e, dy);
    }
  }
  if (T < 2) return;  // no GEMM step: the packed weights are not read
  const unsigned voff = lane * 16;
  const __bf16* a = img + l32 * G::RS + 8 * h;
  WBuf<G> bA, bB;
  wload<G, 0>(rw, voff, bA);
  __syncthreads();
  for (int t = T - 1; t >= 1; --t) {
    f32x16 x[1];
    wgemm<G>(a, rw, voff, bA, bB, x, [&]() { load_epi(t - 1); });
    wload<G, 0>(rw, voff, bA);  // the next step's first range under the element math (unused after the last)
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // every wave is done reading dgh_t's image
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (tile_row(e, h) < B) {
        const float dy = dd[e] + x[0][e];  // dL/dh_t
        if (dh0 && t == 1) stg(rdh0, dy, vh, tile_row(e, 0) * H * 4);
        elem(t - 1, e, dy);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }
}

// hseq[:, 0] = 0: the one slot of hseq the one-launch forward reads and does not write
__global__ __launch_bounds__(THREADS) void zero_h0_kernel(float* __restrict__ hseq, int64_t n, int64_t stride) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < n) hseq[(int64_t)blockIdx.y * stride + i] = 0.f;
}

// FLR_GRU_SEQ=0 (read per call) turns the one-launch form off
inline bool seq_shape_ok(int64_t K, int64_t B, int64_t T, int64_t H) {
  if (flr::knob_off("FLR_GRU_SEQ")) return false;
  // byte offsets within a client's arrays (32 tile rows, 4 H the widest row) stay below 2 GB
  return B <= 32 && H % 32 == 0 && H <= SEQ_HMAX && 32 * (T + 1) * 4 * H < (int64_t)1 << 29;
}

inline bool dims_ok(int64_t K, int64_t B, int64_t T, int64_t H, int64_t t) {
  return K > 0 && B > 0 && T > 0 && H > 0 && t >= 0 && t < T && K * B * H < (int64_t)1 << 31;
}

}  // namespace gru
}  // namespace flr

using namespace flr;

extern "C" int flr_gru_fwd_step(const float* gi, const float* gh, float* hseq, float* gates, int64_t K, int64_t B,
                                int64_t T, int64_t H, int64_t t, void* stream) {
  if (!gi || !gh || !hseq || !gates || !gru::dims_ok(K, B, T, H, t)) return FLR_ERR_ARG;
  const gru::Dims d{(int)K, (int)B, (int)T, (int)H, (int)t};
  const int64_t n = K * B * H;
  hipLaunchKernelGGL(gru::fwd_step_kernel, dim3((unsigned)((n + gru::THREADS - 1) / gru::THREADS)),
                     dim3(gru::THREADS), 0, as_stream(stream), gi, gh, hseq, gates, d);
  return launch_status("gru fwd step");
}

extern "C" int flr_gru_bwd_step(const float* dh, const float* gates, const float* hseq, float* dgh, float* dgi,
                                float* dh_direct, int64_t K, int64_t B, int64_t T, int64_t H, int64_t t,
                                void* stream) {
  if (!dh || !gates || !hseq || !dgh || !dgi || !dh_direct || !gru::dims_ok(K, B, T, H, t)) return FLR_ERR_ARG;
  const gru::Dims d{(int)K, (int)B, (int)T, (int)H, (int)t};
  const int64_t n = K * B * H;
  hipLaunchKernelGGL(gru::bwd_step_kernel, dim3((unsigned)((n + gru::THREADS - 1) / gru::THREADS)),
                     dim3(gru::THREADS), 0, as_stream(stream), dh, gates, hseq, dgh, dgi, dh_direct, d);
  return launch_status("gru bwd step");
}

namespace flr {
namespace gru {
// (waves per workgroup, k-steps per load group); FLR_GRU_FW / FLR_GRU_BW = "NW,G" for A/B timing
// (tools/gru_bench.py); default 8 waves x 2 k-steps for both (C3: fwd 29 us, bwd 27 us per step)
inline int cfg_index(const char* env, int dflt) {
  static const char* names[] = {"4,4", "8,2", "2,8", "8,2s", "8,6", "4,12", "16,3", "", "8,2s"};
  const char* v = flr::knob(env);
  if (v)
    for (int i = 0; i < 9; ++i)
        if (names[i][0] && !strcmp(v, names[i])) return i;
  return dflt;
}
template <bool V8>
inline void launch_fwd(int cfg, dim3 grid, hipStream_t st, const float* gi, const float* whh, const float* bhh,
                       float* hseq, float* gates, const Dims& d, int nub) {
  switch (cfg) {
    case 0: hipLaunchKernelGGL((fwd_fused_kernel<V8, 4, 4>), grid, dim3(256), 0, st, gi, whh, bhh, hseq, gates, d, nub); break;
    case 2: hipLaunchKernelGGL((fwd_fused_kernel<V8, 2, 8>), grid, dim3(128), 0, st, gi, whh, bhh, hseq, gates, d, nub); break;
    case 3: hipLaunchKernelGGL((fwd_fused_kernel<V8, 8, 1, true>), grid, dim3(512), 0, st, gi, whh, bhh, hseq, gates, d, nub); break;
    default: hipLaunchKernelGGL((fwd_fused_kernel<V8, 8, 2>), grid, dim3(512), 0, st, gi, whh, bhh, hseq, gates, d, nub);
  }
}
template <bool V8>
inline void launch_bwd(int cfg, dim3 grid, hipStream_t st, const float* whhT, const float* gates, const float* hseq,
                       float* dgh, float* dgi, float* dh_direct, float* dh0, const Dims& d, int nub) {
  switch (cfg) {
    case 5: hipLaunchKernelGGL((bwd_fused_kernel<V8, 4, 12>), grid, dim3(256), 0, st, whhT, gates, hseq, dgh, dgi, dh_direct, dh0, d, nub); break;
    case 6: hipLaunchKernelGGL((bwd_fused_kernel<V8, 16, 3>), grid, dim3(1024), 0, st, whhT, gates, hseq, dgh, dgi, dh_direct, dh0, d, nub); break;
    case 4: hipLaunchKernelGGL((bwd_fused_kernel<V8, 8, 6>), grid, dim3(512), 0, st, whhT, gates, hseq, dgh, dgi, dh_direct, dh0, d, nub); break;
    case 3: hipLaunchKernelGGL((bwd_fused_kernel<V8, 8, 2, true>), grid, dim3(512), 0, st, whhT, gates, hseq, dgh, dgi, dh_direct, dh0, d, nub); break;
    default: hipLaunchKernelGGL((bwd_fused_kernel<V8, 8, 2>), grid, dim3(512), 0, st, whhT, gates, hseq, dgh, dgi, dh_direct, dh0, d, nub);
  }
}
}  // namespace gru
}  // namespace flr

extern "C" int flr_gru_fwd_fused(const float* gi, const float* whh, const float* bhh, float* hseq, float* gates,
                                 int64_t K, int64_t B, int64_t T, int64_t H, int64_t t, void* stream) {
  return flr_gru_fwd_fused_ex(gi, whh, 0, bhh, hseq, gates, K, B, T, H, t, stream);
}

extern "C" int flr_gru_fwd_fused_ex(const float* gi, const float* whh, int shared_w, const float* bhh, float* hseq,
                                    float* gates, int64_t K, int64_t B, int64_t T, int64_t H, int64_t t,
                                    void* stream) {
  if (!gi || !whh || !bhh || !hseq || !gates || !gru::dims_ok(K, B, T, H, t) || B > 32 || K > 65535)
    return FLR_ERR_ARG;
  const gru::Dims d{(int)K, (int)B, (int)T, (int)H, (int)t, shared_w ? 1 : 0};
  const int nub = (int)((H + 31) / 32);
  const int cfg = gru::cfg_index("FLR_GRU_FW", 1);  // read per call: captured launches keep theirs
  if (H % 8 == 0)
    gru::launch_fwd<true>(cfg, dim3((unsigned)(K * nub)), as_stream(stream), gi, whh, bhh, hseq, gates, d, nub);
  else
    gru::launch_fwd<false>(cfg, dim3((unsigned)(K * nub)), as_stream(stream), gi, whh, bhh, hseq, gates, d, nub);
  return launch_status("gru fwd fused");
}

extern "C" int flr_gru_bwd_fused(const float* whhT, const float* gates, const float* hseq, float* dgh, float* dgi,
                                 float* dh_direct, float* dh0, int64_t K, int64_t B, int64_t T, int64_t H, int64_t t,
                                 void* stream) {
  return flr_gru_bwd_fused_ex(whhT, 0, gates, hseq, dgh, dgi, dh_direct, dh0, K, B, T, H, t, stream);
}

extern "C" int flr_gru_bwd_fused_ex(const float* whhT, int shared_w, const float* gates, const float* hseq,
                                    float* dgh, float* dgi, float* dh_direct, float* dh0, int64_t K, int64_t B,
                                    int64_t T, int64_t H, int64_t t, void* stream) {
  if (!whhT || !gates || !hseq || !dgh || !dgi || !dh_direct || !gru::dims_ok(K, B, T, H, t) || t < 1 || B > 32 ||
      K > 65535)
    return FLR_ERR_ARG;
  const gru::Dims d{(int)K, (int)B, (int)T, (int)H, (int)(t - 1), shared_w ? 1 : 0};
  const int nub = (int)((H + 31) / 32);
  const int cfg = gru::cfg_index("FLR_GRU_BW", 1);
  if (H % 8 == 0)
    gru::launch_bwd<true>(cfg, dim3((unsigned)(K * nub)), as_stream(stream), whhT, gates, hseq, dgh, dgi, dh_direct,
                          dh0, d, nub);
  else
    gru::launch_bwd<false>(cfg, dim3((unsigned)(K * nub)), as_stream(stream), whhT, gates, hseq, dgh, dgi, dh_direct,
                           dh0, d, nub);
  return launch_status("gru bwd fused");
}

extern "C" int flr_gru_seq_supported(int64_t K, int64_t B, int64_t T, int64_t H) {
  return K > 0 && K <= 65535 && B > 0 && T > 0 && H > 0 && gru::seq_shape_ok(K, B, T, H) ? 1 : 0;
}

// A time step of the one-launch form costs about the same at every K up to
// the CU count (one workgroup per client: 20-26 us at H = 256), a per-step
// launch about 7 us per serial round of its K * H/32 one-per-CU workgroups
// (tools/gru_bench.py --seq; profiles/gru_seq): the one launch pays from the
// fourth round on.  FLR_GRU_SEQ=1 takes it at every eligible shape.
extern "C" int flr_gru_seq_preferred(int64_t K, int64_t B, int64_t T, int64_t H) {
  if (!flr_gru_seq_supported(K, B, T, H)) return 0;
  return flr::knob_on("FLR_GRU_SEQ") || K * (H / 32) > 3 * 256 ? 1 : 0;
}

extern "C" int flr_gru_zero_h0(float* hseq, int64_t K, int64_t B, int64_t T, int64_t H, void* stream) {
  if (!hseq || K < 1 || K > 65535 || B < 1 || T < 1 || H < 1 || B * H >= (int64_t)1 << 31) return FLR_ERR_ARG;
  const int64_t n = B * H;
  hipLaunchKernelGGL(gru::zero_h0_kernel, dim3((unsigned)((n + gru::THREADS - 1) / gru::THREADS), (unsigned)K),
                     dim3(gru::THREADS), 0, as_stream(stream), hseq, n, (T + 1) * n);
  return launch_status("gru zero h0");
}

extern "C" int flr_gru_fwd_seq(const float* gi, const float* whhP, int shared_w, const float* bhh, float* hseq,
                               float* gates, int64_t K, int64_t B, int64_t T, int64_t H, void* stream) {
  if (!gi || !whhP || !bhh || !hseq || !gates || !gru::dims_ok(K, B, T, H, 0) || K > 65535) return FLR_ERR_ARG;
  if (!gru::seq_shape_ok(K, B, T, H)) return FLR_ERR_UNSUPPORTED;
  const gru::Dims d{(int)K, (int)B, (int)T, (int)H, 0, shared_w ? 1 : 0};
  switch (H / 32) {
#define FLR_SEQ_CASE(N) \
  case N: hipLaunchKernelGGL(gru::fwd_seq_kernel<32 * N>, dim3((unsigned)K), dim3(64 * N), 0, as_stream(stream), gi, whhP, bhh, hseq, gates, d); break;
    FLR_SEQ_CASE(1) FLR_SEQ_CASE(2) FLR_SEQ_CASE(3) FLR_SEQ_CASE(4) FLR_SEQ_CASE(5) FLR_SEQ_CASE(6) FLR_SEQ_CASE(7)
    FLR_SEQ_CASE(8)
#undef FLR_SEQ_CASE
  }
  return launch_status("gru fwd seq");
}

extern "C" int flr_gru_bwd_seq(const float* whhTP, int shared_w, const float* gates, const float* hseq,
                               const float* dh, float* dgh, float* dgi, float* dh_direct, float* dh0, int64_t K,
                               int64_t B, int64_t T, int64_t H, void* stream) {
  if (!whhTP || !gates || !hseq || !dh || !dgh || !dgi || !dh_direct || !gru::dims_ok(K, B, T, H, 0) || K > 65535)
    return FLR_ERR_ARG;
  if (!gru::seq_shape_ok(K, B, T, H)) return FLR_ERR_UNSUPPORTED;
  const gru::Dims d{(int)K, (int)B, (int)T, (int)H, 0, shared_w ? 1 : 0};
  switch (H / 32) {
#define FLR_SEQ_CASE(N) \
  case N: hipLaunchKernelGGL(gru::bwd_seq_kernel<32 * N>, dim3((unsigned)K), dim3(64 * N), 0, as_stream(stream), whhTP, gates, hseq, dh, dgh, dgi, dh_direct, dh0, d); break;
    FLR_SEQ_CASE(1) FLR_SEQ_CASE(2) FLR_SEQ_CASE(3) FLR_SEQ_CASE(4) FLR_SEQ_CASE(5) FLR_SEQ_CASE(6) FLR_SEQ_CASE(7)
    FLR_SEQ_CASE(8)
#undef FLR_SEQ_CASE
  }
  return launch_status("gru bwd seq");
}

extern "C" int flr_gru_pack(const float* w, int64_t K, int64_t NG, int64_t H, int64_t C, int trans, float* wp,
                            void* stream) {
  if (!w || !wp || K < 1 || K > 65535 || NG < 1 || H < 1 || C < 1 || (trans && NG != 1) ||
      K * NG * H * C >= (int64_t)1 << 31)
    return FLR_ERR_ARG;
  const dim3 grid((unsigned)((C + 127) / 128), (unsigned)(NG * ((H + 31) / 32)), (unsigned)K);
  if (trans)
    hipLaunchKernelGGL(gru::pack_kernel<1>, grid, dim3(256), 0, as_stream(stream), w, (int)NG, (int)H, (int)C, wp);
  else
    hipLaunchKernelGGL(gru::pack_kernel<0>, grid, dim3(256), 0, as_stream(stream), w, (int)NG, (int)H, (int)C, wp);
  return launch_status("gru pack");
}
