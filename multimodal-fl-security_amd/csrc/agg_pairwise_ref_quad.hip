// Reference-exact Krum distances (agg_pairwise_ref.hip), the throughput forms:
// ref_chain_s_kernel<NI, BT> (one wave, x_i in SGPRs) and ref_chain_w_kernel<XL>
// (a 4-wave workgroup sharing x_j through LDS, the default); their launchers at
// the end.
#include "pwref_launch.h"

namespace flr {
namespace pwref {

// K >= 480 (every pair, no tap-major blocks): the throughput form.  Measured
// on gfx950 (tools/hip/pk_rate.hip, profiles/r6_ref/pk_rate.json): at two waves
// per SIMD a plain v_fmac_f32 costs the SIMD 2.3 cycles, a v_sub_f32_dpp about
// 6.6, and packed f32 ops no fewer cycles per element than plain ones; so once
// there are two waves per SIMD to run, the cheapest chain step is a plain
// v_sub_f32 with x_i as an SGPR operand and a plain v_fmac_f32 — 2 SIMD issue
// slots of 2.3 cycles.  A wave holds 8 I rows (wave-uniform, scalar loads) x 64
// J rows (one per lane): 8 chains per lane, each x_j element serves 8 chain
// steps, so the chip's L2 traffic stays at 0.56 B per chain step.
// Operand layout (per segment, quad_transpose_kernel): Xq[c][b][k][e] =
// X[k][8 (r0 + 4 b + e) + c] — per chain c and 4-step block b, the Kp rows'
// 16-B pieces contiguous: lane j's x_j is one coalesced 1-KB load per wave,
// the 8 I rows' block 128 contiguous bytes (two s_load_dwordx16).
//
// One wave: chain c = blockIdx % 8 (the XCD) of tile blockIdx / 8 — J block q,
// I block a: lane l's pairs (NI a + r, 64 q + l), r < NI, valid where i < j < K.
// x_j: one 16-B load per lane and 4-step block, QD blocks in flight (vmcnt, in
// order).  x_i: NI rows x 4 steps x BT blocks per scalar round trip (NI BT / 4
// s_load_dwordx16 into one of two SGPR buffers).  Scalar loads return out of
// order, so a wait for one buffer waits for every scalar load issued: the next
// buffer's loads go out right AFTER the wait for the current one, and the
// latency they can hide is one buffer's compute, 2 NI 4 BT VALU — the reason for
// BT > 1 at NI = 4 (measured: NI = 8, BT = 1 stalled ~650 cycles per buffer,
// profiles/r6_ref/).  Per step the NI chains d = fl(x_i - x_j),
// acc = fma(d, d, acc): the reference's operations in its order.
// one step of the NI chains: plain v_sub_f32 (x_i an SGPR operand) and
// v_fmac_f32, each square one slot behind its difference (inline asm: the
// compiler otherwise SLP-packs the rows into v_pk_* ops whose SGPR pairs cost an
// s_mov per operand).  g0: rows 0-3 of the block (row r's step e at 4 r + e), g1:
// rows 4-7
template <int E>
__device__ __forceinline__ void sgpr_step(float (&acc)[4], const i32x16& g0, const i32x16&, float xjv) {
  float t0, t1;
  asm volatile(
      "v_sub_f32 %[t0], %[s0], %[x]\n\t"
      "v_sub_f32 %[t1], %[s1], %[x]\n\t"
      "v_fmac_f32 %[a0], %[t0], %[t0]\n\t"
      "v_sub_f32 %[t0], %[s2], %[x]\n\t"
      "v_fmac_f32 %[a1], %[t1], %[t1]\n\t"
      "v_sub_f32 %[t1], %[s3], %[x]\n\t"
      "v_fmac_f32 %[a2], %[t0], %[t0]\n\t"
      "v_fmac_f32 %[a3], %[t1], %[t1]\n\t"
      : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [t0] "=&v"(t0), [t1] "=&v"(t1)
      : [s0] "s"(g0[E]), [s1] "s"(g0[4 + E]), [s2] "s"(g0[8 + E]), [s3] "s"(g0[12 + E]), [x] "v"(xjv));
}
// the 8-row step, one text for both operand kinds: CON "s" (x_i in SGPRs) or "v"
// (XL: every lane holds the same value, read from LDS)
#define FLR_STEP8(CON, S0, S1, S2, S3, S4, S5, S6, S7)                                                           \
  float t0, t1;                                                                                                  \
  asm volatile(                                                                                                  \
      "v_sub_f32 %[t0], %[s0], %[x]\n\t"                                                                         \
      "v_sub_f32 %[t1], %[s1], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a0], %[t0], %[t0]\n\t"                                                                       \
      "v_sub_f32 %[t0], %[s2], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a1], %[t1], %[t1]\n\t"                                                                       \
      "v_sub_f32 %[t1], %[s3], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a2], %[t0], %[t0]\n\t"                                                                       \
      "v_sub_f32 %[t0], %[s4], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a3], %[t1], %[t1]\n\t"                                                                       \
      "v_sub_f32 %[t1], %[s5], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a4], %[t0], %[t0]\n\t"                                                                       \
      "v_sub_f32 %[t0], %[s6], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a5], %[t1], %[t1]\n\t"                                                                       \
      "v_sub_f32 %[t1], %[s7], %[x]\n\t"                                                                         \
      "v_fmac_f32 %[a6], %[t0], %[t0]\n\t"                                                                       \
      "v_fmac_f32 %[a7], %[t1], %[t1]\n\t"                                                                       \
      : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [a4] "+v"(acc[4]),           \
        [a5] "+v"(acc[5]), [a6] "+v"(acc[6]), [a7] "+v"(acc[7]), [t0] "=&v"(t0), [t1] "=&v"(t1)                  \
      : [s0] CON(S0), [s1] CON(S1), [s2] CON(S2), [s3] CON(S3), [s4] CON(S4), [s5] CON(S5), [s6] CON(S6),        \
        [s7] CON(S7), [x] "v"(xjv))
template <int E>
__device__ __forceinline__ void sgpr_step(float (&acc)[8], const i32x16& g0, const i32x16& g1, float xjv) {
  FLR_STEP8("s", g0[E], g0[4 + E], g0[8 + E], g0[12 + E], g1[E], g1[4 + E], g1[8 + E], g1[12 + E]);
}
template <int E>
__device__ __forceinline__ void vgpr_step(float (&acc)[8], const f32x4 (&xi)[8], float xjv) {
  FLR_STEP8("v", xi[0][E], xi[1][E], xi[2][E], xi[3][E], xi[4][E], xi[5][E], xi[6][E], xi[7][E]);
}
#undef FLR_STEP8

// The running sums of the previous segments, rows i0 .. i0 + NI - 1 against
// column j of chain c: asm loads and a full wait that ties the loaded values
// (nothing reads them above it), so no compiler-tracked load reaches into the
// loop; the lanes without a pair (i >= j or j >= K) start from 0.
template <int NI>
__device__ __forceinline__ void load_sums(const float* __restrict__ A, int c, int K, int i0, int j, float (&acc)[NI]) {
  static_assert(NI == 4 || NI == 8, "the tied waits below");
#pragma unroll
  for (int r = 0; r < NI; ++r) {
    const float* ap = A + ((int64_t)c * K + i0 + r) * K + (j < K ? j : K - 1);
    asm volatile("global_load_dword %0, %1, off" : "=v"(acc[r]) : "v"(ap) : "memory");
  }
  if constexpr (NI == 4)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) : : "memory");
  else
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                   "+v"(acc[7])
                 :
                 : "memory");
#pragma unroll
  for (int r = 0; r < NI; ++r) acc[r] = (i0 + r < j && j < K) ? acc[r] : 0.f;
}

// FLR_REF_S_ABL (tools build, timing only, wrong results): 1 no x_j loads in the
// loop, 2 no x_i loads, 3 no chain arithmetic
// (tools/ab_build.sh <name> "-DFLR_REF_S_ABL=<n>" agg_pairwise_ref_quad.hip)
#ifndef FLR_REF_S_ABL
#define FLR_REF_S_ABL 0
#endif
template <int NI, int BT>
__global__ __launch_bounds__(64) void ref_chain_s_kernel(const float* __restrict__ Xq, int64_t NB, int64_t Kp, int K,
                                                         int first, float* __restrict__ A) {
  static_assert(NI == 4 || NI == 8, "the step forms above");
  constexpr int NL = NI * BT / 4;  // s_load_dwordx16 per buffer
  static_assert(QD % (2 * BT) == 0, "whole ping-pong pairs of buffers per trip");
  const int c = (int)(blockIdx.x & 7), lane = threadIdx.x;
  const QuadTile qt = find_tile((int)(blockIdx.x >> 3), K, [](int q, int K_) { return quad_ni(q, K_, NI); });
  const int i0 = NI * qt.t, j = QJ * qt.q + lane;
  const float* __restrict__ base = Xq + (int64_t)c * NB * Kp * 4;
  float acc[NI];
  if (first) {
#pragma unroll
    for (int r = 0; r < NI; ++r) acc[r] = 0.f;
  } else {
    load_sums<NI>(A, c, K, i0, j, acc);
  }
  // uniform block pointers advanced per block (the prefetches run up to QD
  // blocks past the segment's last: the workspace's quad slack) and the lane's
  // 32-bit byte offset (the saddr load form)
  const int64_t bb = Kp * 16;  // bytes per block
  const uint32_t voff = (uint32_t)j * 16;
  const char* pjn = reinterpret_cast<const char*>(base);                      // the next x_j block to load
  const char* pin = reinterpret_cast<const char*>(base) + (int64_t)i0 * 16;  // the next x_i buffer
  auto ldj = [&](f32x4& x) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x) : "v"(voff), "s"(pjn) : "memory");
    pjn += bb;
    asm volatile("" : "+s"(pjn));  // one running pointer, not QD precomputed ones
  };
  // buffer: block u's 4-row groups at buf[u NI / 4 ..]
  auto ldi = [&](i32x16(&buf)[NL]) {
    const char* pu = pin;
#pragma unroll
    for (int u = 0; u < BT; ++u) {
#pragma unroll
      for (int h = 0; h < NI / 4; ++h)
        asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(buf[u * (NI / 4) + h]) : "s"(pu), "n"(64 * h) : "memory");
      pu += bb;
      asm volatile("" : "+s"(pu));
    }
    pin = pu;
  };
  f32x4 xj[QD];
  i32x16 xa[NL], xb[NL];
#pragma unroll
  for (int u = 0; u < QD; ++u) ldj(xj[u]);
  ldi(xa);
  // a buffer's BT blocks: x_i(buffer) landed, then the next buffer issued;
  // per block x_j(b) landed, its 4 steps, x_j(b + QD) issued into the freed registers
  auto trip = [&](auto U0, const i32x16(&cur)[NL], i32x16(&nxt)[NL]) {
    constexpr int u0 = decltype(U0)::value;
    // the scalar loads into `cur` landed: never reuse or read their SGPRs without this wait
    if (FLR_REF_S_ABL != 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (FLR_REF_S_ABL != 2) ldi(nxt);
#pragma unroll
    for (int v = 0; v < BT; ++v) {
      f32x4& x = xj[u0 + v];
      if (FLR_REF_S_ABL != 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QD - 1) : "memory");
      asm volatile("" : "+v"(x));  // x arrived at the wait above
      const i32x16& g0 = cur[v * (NI / 4)];
      const i32x16& g1 = cur[v * (NI / 4) + (NI / 4) - 1];
      if (FLR_REF_S_ABL != 3) {
        sgpr_step<0>(acc, g0, g1, x[0]);
        sgpr_step<1>(acc, g0, g1, x[1]);
        sgpr_step<2>(acc, g0, g1, x[2]);
        sgpr_step<3>(acc, g0, g1, x[3]);
      }
      if (FLR_REF_S_ABL != 1) ldj(x);
    }
  };
  for (int64_t b0 = 0; b0 < NB; b0 += QD)
    static_for(
        [&](auto P) {
          constexpr int p = decltype(P)::value;
          trip(std::integral_constant<int, 2 * BT * p>{}, xa, xb);
          trip(std::integral_constant<int, 2 * BT * p + BT>{}, xb, xa);
        },
        std::make_integer_sequence<int, QD / (2 * BT)>{});
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int r = 0; r < NI; ++r) {
    const int i = i0 + r;
    if (i < j && j < K) A[((int64_t)c * K + i) * K + j] = acc[r];
  }
}

// The workgroup form (default for the throughput path): 4 waves = 4 I blocks
// (32 rows) of one J block share its x_j through LDS.  Measured, the one-wave
// form above is bound by its x_j stream, not its arithmetic (without any chain
// arithmetic it ran 21.5 of 22.1 ms at K = 512, P = 2M, profiles/r6_sgpr/): its
// waves drift apart, the L2 no longer serves one J block to the many waves that
// read it, and the chip streams ~7.7 TB/s.  Here a 4-wave workgroup stages each
// chunk of WCB blocks of its J rows (WCB KB) once by LDS-DMA into a ring of WNS
// stages — one barrier per chunk keeps its waves together — and each lane reads
// its row's 16-B piece per block with ds_read_b128 (1 KB per wave: ~4 LDS cycles
// per 64 VALU).  x_i as above (SGPR operands, one block ahead).
constexpr int WCB = 8;  // 4-step blocks per staged chunk (WCB KB: one 1-KB DMA per block)
constexpr int WNS = 4;  // ring stages
static_assert(WCB % 8 == 0 && (XC_GROUP / 4) % WCB == 0, "two DMAs per wave per chunk; whole chunks per segment");

// XL: x_i staged through LDS too (the group's 32 I rows, 512 B per block) and
// read as broadcast ds_read_b128 into VGPR operands — no scalar loads (their
// round trip, ~600 cycles under load, bounded the SGPR form: one block's
// compute is all a scalar prefetch can hide, as they complete out of order)
template <bool XL>
__global__ __launch_bounds__(256, 3) void ref_chain_w_kernel(const float* __restrict__ Xq, int64_t NB, int64_t Kp,
                                                             int K, int first, float* __restrict__ A) {
  constexpr int SJ = WCB * QJ * 16;              // x_j bytes per stage
  constexpr int SI = XL ? WCB * 32 * 16 : 0;     // x_i bytes per stage
  constexpr int NDMA = XL ? 3 : 2;               // DMA instructions per wave per chunk
  __shared__ __attribute__((aligned(16))) float xs[WNS * (SJ + SI) / 4];  // [stage]{[block][row][4] x_j, x_i}
  const int c = (int)(blockIdx.x & 7), lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform (SGPR operands)
  const QuadTile qt = find_tile((int)(blockIdx.x >> 3), K, [](int q, int K_) { return wg_groups(q, K_); });
  const int t = qt.t, q = qt.q;
  // this wave's I block; past the J block's last one (a ragged group) the wave
  // still stages and meets every barrier, and stores nothing
  const int a = 4 * t + wave, na = quad_ni(q, K, 8);
  const bool live = a < na;
  const int i0 = 8 * (live ? a : na - 1), j = QJ * q + lane;
  const float* __restrict__ base = Xq + (int64_t)c * NB * Kp * 4;
  float acc[8];
  if (first || !live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.f;
  } else {
    load_sums<8>(A, c, K, i0, j, acc);
  }
  const int64_t bb = Kp * 16;   // bytes per block
  const int64_t nch = NB / WCB;  // chunks in the segment
  // staging: wave w moves x_j blocks 2w, 2w + 1 of a chunk (the J block's 64
  // rows, 1 KB contiguous each) and (XL) the x_i of the same two blocks (the
  // group's 32 rows, 512 B each: lanes 0-31 block 2w, 32-63 block 2w + 1)
  const char* jsrc = reinterpret_cast<const char*>(base) + (int64_t)(QJ * q) * 16;
  const char* isrc = reinterpret_cast<const char*>(base) + (int64_t)(32 * t) * 16;
  const uint32_t vj = (uint32_t)lane * 16;
  const uint32_t vi = (uint32_t)(((lane >> 5) * Kp + (lane & 31)) * 16);
  const uint32_t lds0 = (uint32_t)(uintptr_t)xs;
  auto dma = [&](int64_t ch) {
    const int64_t cc = ch < nch ? ch : nch - 1;  // past the last chunk: the last again (nothing reads it)
    const uint32_t sb = lds0 + (uint32_t)((int)(ch % WNS) * (SJ + SI));
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int blk = 2 * wave + v;
      const char* src = jsrc + (cc * WCB + blk) * bb;
      const uint32_t m = sb + (uint32_t)(blk * QJ * 16);
      // M0 written in the statement that reads it; nothing else in the kernel reads M0
      asm volatile("s_mov_b32 m0, %[m]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v], %[s] offset:0"
                   :
                   : [m] "s"(m), [v] "v"(vj), [s] "s"(src)
                   : "memory");
    }
    if constexpr (XL) {
      const char* src = isrc + (cc * WCB + 2 * wave) * bb;
      const uint32_t m = sb + SJ + (uint32_t)(2 * wave * 32 * 16);
      asm volatile("s_mov_b32 m0, %[m]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v], %[s] offset:0"
                   :
                   : [m] "s"(m), [v] "v"(vi), [s] "s"(src)
                   : "memory");
    }
  };
  const char* pin = reinterpret_cast<const char*>(base) + (int64_t)i0 * 16;  // the next x_i block (SGPR form)
  auto ldi = [&](i32x16& lo, i32x16& hi) {
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40" : "=s"(lo), "=s"(hi) : "s"(pin) : "memory");
    pin += bb;
    asm volatile("" : "+s"(pin));
  };
  auto rdj = [&](f32x4& x, uint32_t addr, auto U) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x) : "v"(addr), "n"(decltype(U)::value * QJ * 16) : "memory");
  };
  // XL: row r of this wave's 8 at byte 16 (32 u + 8 wave + r) of the stage's x_i
  // (the same address in every lane: a broadcast)
  auto rdi = [&](f32x4(&x)[8], uint32_t addr, auto U) {
#pragma unroll
    for (int r = 0; r < 8; ++r)
      asm volatile("ds_read_b128 %0, %1 offset:%2"
                   : "=v"(x[r])
                   : "v"(addr), "n"(SJ + decltype(U)::value * 32 * 16 + 16 * r)
                   : "memory");
  };
  i32x16 al, ah, bl, bh;
  f32x4 j0, j1, ia[8], ib[8];
#pragma unroll
  for (int p = 0; p < WNS - 1; ++p) dma(p);
  if constexpr (!XL) ldi(al, ah);
  // block u of chunk ch: x_i(b) and x_j(b) landed; x_i(b + 1) issued (the SGPR
  // form: always; XL: inside the chunk, like x_j(b + 1)); the block's 4 steps
  auto body = [&](auto U, uint32_t sbase, uint32_t ibase, f32x4& xc, f32x4& xn, const i32x16& cl,
                  const i32x16& ch_, i32x16& nl, i32x16& nh, f32x4(&ic)[8], f32x4(&in)[8]) {
    constexpr int u = decltype(U)::value;
    if constexpr (XL) {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(xc), "+v"(ic[0]), "+v"(ic[1]), "+v"(ic[2]), "+v"(ic[3]), "+v"(ic[4]), "+v"(ic[5]),
                     "+v"(ic[6]), "+v"(ic[7])
                   :
                   : "memory");
      if constexpr (u + 1 < WCB) {
        rdj(xn, sbase, std::integral_constant<int, u + 1>{});
        rdi(in, ibase, std::integral_constant<int, u + 1>{});
      }
      vgpr_step<0>(acc, ic, xc[0]);
      vgpr_step<1>(acc, ic, xc[1]);
      vgpr_step<2>(acc, ic, xc[2]);
      vgpr_step<3>(acc, ic, xc[3]);
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xc) : : "memory");
      ldi(nl, nh);
      if constexpr (u + 1 < WCB) rdj(xn, sbase, std::integral_constant<int, u + 1>{});
      sgpr_step<0>(acc, cl, ch_, xc[0]);
      sgpr_step<1>(acc, cl, ch_, xc[1]);
      sgpr_step<2>(acc, cl, ch_, xc[2]);
      sgpr_step<3>(acc, cl, ch_, xc[3]);
    }
  };
  static_assert(WCB % 2 == 0, "x_i / x_j ping-pong");
  for (int64_t ch = 0; ch < nch; ++ch) {
    // this wave's DMAs of chunk ch landed (the younger ones: chunks ch + 1 ..
    // ch + WNS - 2), then every wave's (the barrier), which also marks every
    // wave done with chunk ch - 1, whose stage the next DMA refills
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NDMA * (WNS - 2)) : "memory");
    dma(ch + WNS - 1);
    const uint32_t st = lds0 + (uint32_t)((int)(ch % WNS) * (SJ + SI));
    const uint32_t sbase = st + vj;
    const uint32_t ibase = st + (uint32_t)(wave * 8 * 16);  // uniform: a broadcast address
    rdj(j0, sbase, std::integral_constant<int, 0>{});
    if constexpr (XL) rdi(ia, ibase, std::integral_constant<int, 0>{});
    static_for(
        [&](auto P) {
          constexpr int p = decltype(P)::value;
          body(std::integral_constant<int, 2 * p>{}, sbase, ibase, j0, j1, al, ah, bl, bh, ia, ib);
          body(std::integral_constant<int, 2 * p + 1>{}, sbase, ibase, j1, j0, bl, bh, al, ah, ib, ia);
        },
        std::make_integer_sequence<int, WCB / 2>{});
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = i0 + r;
      if (i < j && j < K) A[((int64_t)c * K + i) * K + j] = acc[r];
    }
  }
}

int launch_ref_chain_s(int ni, const float* Xq, int64_t NB, int64_t Kp, int64_t K, int first, float* A, hipStream_t st) {
  auto kern = ni == 8 ? ref_chain_s_kernel<8, 1> : ref_chain_s_kernel<4, 2>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(8 * quad_ntiles((int)K, ni))), dim3(64), 0, st, Xq, NB, Kp, (int)K, first,
                     A);
  return launch_status("ref_chain_s_kernel");
}

int launch_ref_chain_w(bool xl, const float* Xq, int64_t NB, int64_t Kp, int64_t K, int first, float* A,
                       hipStream_t st) {
  auto kern = xl ? ref_chain_w_kernel<true> : ref_chain_w_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(8 * wg_ntiles((int)K))), dim3(256), 0, st, Xq, NB, Kp, (int)K, first, A);
  return launch_status("ref_chain_w_kernel");
}

}  // namespace pwref
}  // namespace flr
