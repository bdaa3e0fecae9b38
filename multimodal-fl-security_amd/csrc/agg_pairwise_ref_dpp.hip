// Reference-exact Krum distances (agg_pairwise_ref.hip), the DPP chain forms:
// one wave per workgroup, one chain per lane, x_j from an LDS-DMA ring and x_i
// by DPP broadcast — ref_chain_kernel (the default below K = 480 and for tile
// ranges), ref_chain_dead_kernel<DM> (a dead region's two streams) and
// ref_chain2_kernel (two chains per lane, opt-in); their launchers at the end.
// Tools builds: tools/ab_build.sh <name> "-DFLR_REF_ABL=<n>" agg_pairwise_ref_dpp.hip
// (-DFLR_REF_NSTAGE=<n>: the ring's stages, within the static_asserts below).
#include "pwref_launch.h"

namespace flr {
namespace pwref {

#ifndef FLR_REF_NSTAGE
#define FLR_REF_NSTAGE 8
#endif
constexpr int NSTAGE = FLR_REF_NSTAGE;    // LDS ring = the loop's unroll (DMA NSTAGE - 1 chunks ahead)
constexpr int STAGE = SROWS * CS;         // floats per stage (5 KB)
static_assert(NSTAGE % 2 == 0 && NSTAGE >= 4, "two register buffers");
static_assert(XC_GROUP % (NSTAGE * CS) == 0, "whole loop trips inside a padded stream");
static_assert((NSTAGE - 1) * CS * 4 <= XC_SLACK, "the prefetch past a stream stays inside the slack");
static_assert((NSTAGE - 1) * STAGE * 4 < 65536, "ds_read_b128's 16-bit offset reaches every stage");
static_assert(NSTAGE * STAGE * 4 > 163840 / 5, "LDS caps the CU at four workgroups: one wave per SIMD");
template <bool DIAG>
struct Staging {
  static constexpr int DPW = (DIAG ? SROWS : JW) / RPD;  // DMA instructions per chunk (5 | 4)
  static constexpr int OPB = DPW + 1;                   // vector-memory ops per body: the DMAs, then x_i
  static_assert((NSTAGE - 2) * OPB + 1 < 64, "vmcnt counts to 63");
};

// One chunk (CS = 64 steps) of a lane's chain: step S subtracts its x_j from
// x_i's step S, which lane S / 4 of each 16-lane row holds (component S % 4) and
// a DPP row_newbcast hands to every lane, folded into the subtraction
// (v_sub_f32_dpp), then acc = fma(d, d, acc).  Inline asm fixes the order
// (the subtraction of step S + 2 in the gap before the dependent fma of step
// S; blocks of 16 steps, three rotating temporaries).  The s_nop before the
// first block covers the DPP read-after-VALU-write hazard on x_i (the compiler
// cannot see a DPP inside asm; the later blocks follow asm that writes only the
// temporaries and acc).
// FLR_REF_ABL (tools build, timing only, wrong results): 1 plain v_sub instead
// of the DPP broadcast, 2 no LDS reads, 3 no DMA / x_i loads, 5 no chain
// arithmetic
#ifndef FLR_REF_ABL
#define FLR_REF_ABL 0
#endif
#if FLR_REF_ABL == 1
#define FLR_SUBJ(T, X, J, L) "v_sub_f32 %[" #T "], %[" #X "], %[" #J "]\n\t"
#else
#define FLR_SUBJ(T, X, J, L) \
  "v_sub_f32_dpp %[" #T "], %[" #X "], %[" #J "] row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
#endif
#define FLR_SQ(T) "v_fmac_f32 %[acc], %[" #T "], %[" #T "]\n\t"
#define FLR_CHAIN16(A, B, C, D, NOP)                                                                  \
  NOP FLR_SUBJ(t0, x0, j0, A) FLR_SUBJ(t1, x1, j1, A) FLR_SQ(t0) FLR_SUBJ(t2, x2, j2, A) FLR_SQ(t1)   \
      FLR_SUBJ(t0, x3, j3, A) FLR_SQ(t2) FLR_SUBJ(t1, x0, j4, B) FLR_SQ(t0) FLR_SUBJ(t2, x1, j5, B)   \
      FLR_SQ(t1) FLR_SUBJ(t0, x2, j6, B) FLR_SQ(t2) FLR_SUBJ(t1, x3, j7, B) FLR_SQ(t0)                \
      FLR_SUBJ(t2, x0, j8, C) FLR_SQ(t1) FLR_SUBJ(t0, x1, j9, C) FLR_SQ(t2) FLR_SUBJ(t1, x2, j10, C)  \
      FLR_SQ(t0) FLR_SUBJ(t2, x3, j11, C) FLR_SQ(t1) FLR_SUBJ(t0, x0, j12, D) FLR_SQ(t2)              \
      FLR_SUBJ(t1, x1, j13, D) FLR_SQ(t0) FLR_SUBJ(t2, x2, j14, D) FLR_SQ(t1) FLR_SUBJ(t0, x3, j15, D) \
      FLR_SQ(t2) FLR_SQ(t0)
#define FLR_CHAIN_BLOCK(b, A, B, C, D, NOP)                                                                \
  asm volatile(FLR_CHAIN16(A, B, C, D, NOP)                                                                \
               : [acc] "+v"(acc), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2)                        \
               : [x0] "v"(xv[0]), [x1] "v"(xv[1]), [x2] "v"(xv[2]), [x3] "v"(xv[3]), [j0] "v"(v[4 * (b) + 0][0]), [j1] "v"(v[4 * (b) + 0][1]), [j2] "v"(v[4 * (b) + 0][2]), [j3] "v"(v[4 * (b) + 0][3]), [j4] "v"(v[4 * (b) + 1][0]), [j5] "v"(v[4 * (b) + 1][1]), [j6] "v"(v[4 * (b) + 1][2]), [j7] "v"(v[4 * (b) + 1][3]), [j8] "v"(v[4 * (b) + 2][0]), [j9] "v"(v[4 * (b) + 2][1]), [j10] "v"(v[4 * (b) + 2][2]), [j11] "v"(v[4 * (b) + 2][3]), [j12] "v"(v[4 * (b) + 3][0]), [j13] "v"(v[4 * (b) + 3][1]), [j14] "v"(v[4 * (b) + 3][2]), [j15] "v"(v[4 * (b) + 3][3]))
__device__ __forceinline__ float chain_chunk(f32x4 xv, const f32x4 (&v)[NQ], float acc) {
  static_assert(NQ == 16, "four blocks of 16 steps");
  float t0, t1, t2;
  FLR_CHAIN_BLOCK(0, 0, 1, 2, 3, "s_nop 1\n\t");
  FLR_CHAIN_BLOCK(1, 4, 5, 6, 7, "");
  FLR_CHAIN_BLOCK(2, 8, 9, 10, 11, "");
  FLR_CHAIN_BLOCK(3, 12, 13, 14, 15, "");
  return acc;
}
#undef FLR_CHAIN_BLOCK
#undef FLR_CHAIN16
#undef FLR_SQ
#undef FLR_SUBJ

// Two chains per lane (K >= 256, off-diagonal tiles, ref_chain2_kernel): the
// lane's pairs (i, j) and (i + 4, j) share the staged x_j; per step two
// v_sub_f32_dpp (x_i and x_i2 broadcast by row_newbcast, as above) and two
// v_fmac, the previous step's squares one slot behind its subtraction.
#define FLR_STEP2(XA, XB, J, L, TA, TB, PA, PB) \
  "v_sub_f32_dpp %[" #TA "], %[" #XA "], %[" #J "] row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t" \
  "v_sub_f32_dpp %[" #TB "], %[" #XB "], %[" #J "] row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t" \
  "v_fmac_f32 %[acc], %[" #PA "], %[" #PA "]\n\t" \
  "v_fmac_f32 %[acc2], %[" #PB "], %[" #PB "]\n\t"
#define FLR_STEP2_FIRST(XA, XB, J, L, TA, TB) \
  "v_sub_f32_dpp %[" #TA "], %[" #XA "], %[" #J "] row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t" \
  "v_sub_f32_dpp %[" #TB "], %[" #XB "], %[" #J "] row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
#define FLR_CHAIN16_2(A, B, C, D, NOP) \
  NOP \
  FLR_STEP2_FIRST(x0, y0, j0, A, a0, b0) \
  FLR_STEP2(x1, y1, j1, A, a1, b1, a0, b0) FLR_STEP2(x2, y2, j2, A, a0, b0, a1, b1) \
  FLR_STEP2(x3, y3, j3, A, a1, b1, a0, b0) FLR_STEP2(x0, y0, j4, B, a0, b0, a1, b1) \
  FLR_STEP2(x1, y1, j5, B, a1, b1, a0, b0) FLR_STEP2(x2, y2, j6, B, a0, b0, a1, b1) \
  FLR_STEP2(x3, y3, j7, B, a1, b1, a0, b0) FLR_STEP2(x0, y0, j8, C, a0, b0, a1, b1) \
  FLR_STEP2(x1, y1, j9, C, a1, b1, a0, b0) FLR_STEP2(x2, y2, j10, C, a0, b0, a1, b1) \
  FLR_STEP2(x3, y3, j11, C, a1, b1, a0, b0) FLR_STEP2(x0, y0, j12, D, a0, b0, a1, b1) \
  FLR_STEP2(x1, y1, j13, D, a1, b1, a0, b0) FLR_STEP2(x2, y2, j14, D, a0, b0, a1, b1) \
  FLR_STEP2(x3, y3, j15, D, a1, b1, a0, b0) \
  "v_fmac_f32 %[acc], %[a1], %[a1]\n\t" \
  "v_fmac_f32 %[acc2], %[b1], %[b1]\n\t"
#define FLR_CHAIN_BLOCK2(b, A, B, C, D, NOP)                                                                   \
  asm volatile(FLR_CHAIN16_2(A, B, C, D, NOP)                                                                 \
               : [acc] "+v"(acc), [acc2] "+v"(acc2), [a0] "=&v"(a0), [b0] "=&v"(b0), [a1] "=&v"(a1),          \
                 [b1] "=&v"(b1)                                                                              \
               : [x0] "v"(xv[0]), [x1] "v"(xv[1]), [x2] "v"(xv[2]), [x3] "v"(xv[3]), [y0] "v"(yv[0]),           \
                 [y1] "v"(yv[1]), [y2] "v"(yv[2]), [y3] "v"(yv[3]), [j0] "v"(v[4 * (b) + 0][0]),              \
                 [j1] "v"(v[4 * (b) + 0][1]), [j2] "v"(v[4 * (b) + 0][2]), [j3] "v"(v[4 * (b) + 0][3]),        \
                 [j4] "v"(v[4 * (b) + 1][0]), [j5] "v"(v[4 * (b) + 1][1]), [j6] "v"(v[4 * (b) + 1][2]),        \
                 [j7] "v"(v[4 * (b) + 1][3]), [j8] "v"(v[4 * (b) + 2][0]), [j9] "v"(v[4 * (b) + 2][1]),        \
                 [j10] "v"(v[4 * (b) + 2][2]), [j11] "v"(v[4 * (b) + 2][3]), [j12] "v"(v[4 * (b) + 3][0]),     \
                 [j13] "v"(v[4 * (b) + 3][1]), [j14] "v"(v[4 * (b) + 3][2]), [j15] "v"(v[4 * (b) + 3][3]))
__device__ __forceinline__ void chain_chunk2(f32x4 xv, f32x4 yv, const f32x4 (&v)[NQ], float& acc, float& acc2) {
  float a0, b0, a1, b1;
  FLR_CHAIN_BLOCK2(0, 0, 1, 2, 3, "s_nop 1\n\t");
  FLR_CHAIN_BLOCK2(1, 4, 5, 6, 7, "");
  FLR_CHAIN_BLOCK2(2, 8, 9, 10, 11, "");
  FLR_CHAIN_BLOCK2(3, 12, 13, 14, 15, "");
}
#undef FLR_CHAIN_BLOCK2
#undef FLR_CHAIN16_2
#undef FLR_STEP2_FIRST
#undef FLR_STEP2
// A dead region's chunk: CS live steps and the dead steps between them, in
// the chain's order (DeadPlan: periods of the taps 8 .. 0).  DM: the block's
// dead-tap mask.  Live steps as chain_chunk (the subtraction two live steps
// ahead of its fma, three temporaries).  A dead step is acc = fma(T, T, acc):
// T from the stage's dead stream by ds_read_b128 of an address every mixed
// lane shares (a broadcast); the other lanes read zeros instead (ta: their
// address is the zero block), which leaves their sums as they are.  RQ reads
// in flight, waited by count (LDS returns in order; the next chunk's x_j reads
// are older than every one of them).
template <int DM>
struct DeadPat {
  static constexpr int ND = __builtin_popcount(DM & 0x1ff), NL = 9 - ND;
  static_assert(ND > 0 && NL > 0 && CS % NL == 0, "whole periods per chunk");
  static constexpr int PPC = CS / NL;   // periods per chunk
  static constexpr int TCH = PPC * ND;  // dead steps per chunk
  static_assert(TCH % 4 == 0, "16-B reads of the dead stream");
  static constexpr int NQT = TCH / 4;
  static constexpr int NT = (TCH * 4 + 1023) / 1024;  // 1-KB DMA instructions per chunk
  static constexpr bool dead_at(int w) { return (DM >> (8 - w)) & 1; }  // position w of a period: tap 8 - w
  static constexpr int dead_before(int w) {
    int n = 0;
    for (int x = 0; x < w; ++x) n += dead_at(x) ? 1 : 0;
    return n;
  }
};
#define FLR_FMA(x) "v_fmac_f32 %[acc], %[" #x "], %[" #x "]\n\t"
#define FLR_SUB(dd, x, j, L) \
  "v_sub_f32_dpp %[" #dd "], %[" #x "], %[" #j "] row_newbcast:%[" #L "] row_mask:0xf bank_mask:0xf\n\t"
template <int DM>
__device__ __forceinline__ float dead_chunk(f32x4 xv, const f32x4 (&v)[NQ], float acc, uint32_t ta) {
  using Pt = DeadPat<DM>;
  static_assert(DM == 0x1EF || DM == 0x04F, "the period statements below");
  constexpr int ND = Pt::ND, NQT = Pt::NQT;
  constexpr int RQ = NQT < 20 ? NQT : (DM == 0x1EF ? 14 : 20);  // 16-B reads of the dead stream in flight
  f32x4 tq[RQ];
  float d[3];
  auto readq = [&tq, &ta](auto Q) {  // (captures named: asm operands alone do not capture)
    constexpr int q = decltype(Q)::value;
    (void)tq, (void)ta;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(tq[q % RQ]) : "v"(ta), "n"(16 * q) : "memory");
  };
  static_for([&readq](auto Q) { readq(Q); }, std::make_integer_sequence<int, RQ>{});
  // the first two live steps' differences; the s_nop covers the DPP
  // read-after-write hazard on x_i (chain_chunk)
  asm volatile("s_nop 1\n\t" FLR_SUB(da, x0, j0, L) FLR_SUB(db, x1, j1, L)
               : [da] "=&v"(d[0]), [db] "=&v"(d[1])
               : [x0] "v"(xv[0]), [x1] "v"(xv[1]), [j0] "v"(v[0][0]), [j1] "v"(v[0][1]), [L] "n"(0));
  // One statement per G periods (the compiler's hazard pass puts an s_nop
  // between dependent statements: single-instruction ones double the count).
  // Group pg: dead values n0 .. n0 + G ND - 1 of the chunk (n / 4: the read,
  // n % 4: its component), waited for at the group's start by count: the
  // reads issued so far end with quad `last`.
  constexpr int G = DM == 0x1EF ? 2 : 1;
  static_assert(Pt::PPC % G == 0, "whole groups per chunk");
  static_for(
      [&tq, &d, &acc, &readq, &xv, &v](auto PP) {
        constexpr int pg = decltype(PP)::value, p = G * pg, n0 = ND * p;
        (void)tq, (void)d, (void)acc, (void)xv, (void)v;
        constexpr int done = n0 / 4, last = (done + RQ < NQT ? done + RQ : NQT) - 1, need = (n0 + G * ND - 1) / 4;
        constexpr int cnt = last - need < 15 ? last - need : 15;
        static_assert(need <= last, "the group's reads were issued");
#define FLR_T(n) tq[((n0 + (n)) / 4) % RQ][(n0 + (n)) % 4]
#define FLR_T8(a, b) [t##a##0] "v"(FLR_T(b + 0)), [t##a##1] "v"(FLR_T(b + 1)), [t##a##2] "v"(FLR_T(b + 2)), \
                     [t##a##3] "v"(FLR_T(b + 3)), [t##a##4] "v"(FLR_T(b + 4)), [t##a##5] "v"(FLR_T(b + 5)), \
                     [t##a##6] "v"(FLR_T(b + 6)), [t##a##7] "v"(FLR_T(b + 7))
        if constexpr (DM == 0x1EF) {  // D D D D L D D D D, twice: live steps S = p and S + 1
          constexpr int S = p, N = S + 2 < CS ? S + 2 : 0;  // the differences two live steps ahead
          if constexpr (S + 2 < CS)
            asm volatile("s_waitcnt lgkmcnt(%[w])\n\t" FLR_FMA(ta0) FLR_FMA(ta1) FLR_FMA(ta2) FLR_FMA(ta3) FLR_FMA(d0)
                             FLR_SUB(n0, x0, j0, L0) FLR_FMA(ta4) FLR_FMA(ta5) FLR_FMA(ta6) FLR_FMA(ta7)
                                 FLR_FMA(tb0) FLR_FMA(tb1) FLR_FMA(tb2) FLR_FMA(tb3) FLR_FMA(d1)
                                     FLR_SUB(d0, x1, j1, L1) FLR_FMA(tb4) FLR_FMA(tb5) FLR_FMA(tb6) FLR_FMA(tb7)
                         : [acc] "+v"(acc), [d0] "+v"(d[S % 3]), [d1] "+v"(d[(S + 1) % 3]), [n0] "=&v"(d[(S + 2) % 3])
                         : [x0] "v"(xv[N % 4]), [j0] "v"(v[N / 4][N % 4]), [L0] "n"(N / 4), [x1] "v"(xv[(N + 1) % 4]),
                           [j1] "v"(v[(N + 1) / 4][(N + 1) % 4]), [L1] "n"((N + 1) / 4), [w] "n"(cnt), FLR_T8(a, 0),
                           FLR_T8(b, 8));
          else
            asm volatile("s_waitcnt lgkmcnt(%[w])\n\t" FLR_FMA(ta0) FLR_FMA(ta1) FLR_FMA(ta2) FLR_FMA(ta3) FLR_FMA(d0)
                             FLR_FMA(ta4) FLR_FMA(ta5) FLR_FMA(ta6) FLR_FMA(ta7) FLR_FMA(tb0) FLR_FMA(tb1)
                                 FLR_FMA(tb2) FLR_FMA(tb3) FLR_FMA(d1) FLR_FMA(tb4) FLR_FMA(tb5) FLR_FMA(tb6)
                                     FLR_FMA(tb7)
                         : [acc] "+v"(acc)
                         : [d0] "v"(d[S % 3]), [d1] "v"(d[(S + 1) % 3]), [w] "n"(cnt), FLR_T8(a, 0), FLR_T8(b, 8));
        } else {  // L L D L L D D D D: live steps S .. S + 3, S = 4 p; temporaries da, db, dc = d[S % 3] ..
          constexpr int S = 4 * p;
          float &da = d[S % 3], &db = d[(S + 1) % 3], &dc = d[(S + 2) % 3];
          if constexpr (S + 4 < CS)
            asm volatile("s_waitcnt lgkmcnt(%[w])\n\t" FLR_FMA(da) FLR_SUB(dc, x2, j2, L0) FLR_FMA(db)
                             FLR_SUB(da, x3, j3, L0) FLR_FMA(t0) FLR_FMA(dc) FLR_SUB(db, x0, j4, L1) FLR_FMA(da)
                                 FLR_SUB(dc, x1, j5, L1) FLR_FMA(t1) FLR_FMA(t2) FLR_FMA(t3) FLR_FMA(t4)
                         : [acc] "+v"(acc), [da] "+v"(da), [db] "+v"(db), [dc] "+v"(dc)
                         : [x0] "v"(xv[0]), [x1] "v"(xv[1]), [x2] "v"(xv[2]), [x3] "v"(xv[3]), [j2] "v"(v[p][2]),
                           [j3] "v"(v[p][3]), [j4] "v"(v[p + 1 < NQ ? p + 1 : p][0]),
                           [j5] "v"(v[p + 1 < NQ ? p + 1 : p][1]), [L0] "n"(p), [L1] "n"(p + 1), [w] "n"(cnt),
                           [t0] "v"(FLR_T(0)), [t1] "v"(FLR_T(1)), [t2] "v"(FLR_T(2)), [t3] "v"(FLR_T(3)),
                           [t4] "v"(FLR_T(4)));
          else  // the chunk's last period: no step past it
            asm volatile("s_waitcnt lgkmcnt(%[w])\n\t" FLR_FMA(da) FLR_SUB(dc, x2, j2, L0) FLR_FMA(db)
                             FLR_SUB(da, x3, j3, L0) FLR_FMA(t0) FLR_FMA(dc) FLR_FMA(da) FLR_FMA(t1) FLR_FMA(t2)
                                 FLR_FMA(t3) FLR_FMA(t4)
                         : [acc] "+v"(acc), [da] "+v"(da), [db] "+v"(db), [dc] "+v"(dc)
                         : [x2] "v"(xv[2]), [x3] "v"(xv[3]), [j2] "v"(v[p][2]), [j3] "v"(v[p][3]), [L0] "n"(p),
                           [w] "n"(cnt), [t0] "v"(FLR_T(0)), [t1] "v"(FLR_T(1)), [t2] "v"(FLR_T(2)),
                           [t3] "v"(FLR_T(3)), [t4] "v"(FLR_T(4)));
        }
#undef FLR_T8
#undef FLR_T
        // the reads this group used up are free: the next RQ ahead into them
        static_for(
            [&readq](auto E) {
              constexpr int q = done + decltype(E)::value;
              if constexpr (4 * q + 3 < n0 + G * ND && q + RQ < NQT) readq(std::integral_constant<int, q + RQ>{});
            },
            std::make_integer_sequence<int, (G * ND + 3) / 4 + 1>{});
      },
      std::make_integer_sequence<int, Pt::PPC / G>{});
  return acc;
}
#undef FLR_SUB
#undef FLR_FMA

// One segment of steps of one tile (one wave): chain c of each lane's pair; the
// running chain sums in A[c][min(i,j)][max(i,j)] (first: start from 0).
//
// Body ch (stage u = ch % NSTAGE, static in the unrolled loop):
//   wait  DMA(ch + 1) and x_i(ch) landed (counted vmcnt: the DMA's LDS writes
//         are then visible to this wave), the ds_reads of chunk ch landed
//         (lgkmcnt(0): stage (ch - 1) % NSTAGE is free)
//   issue DMA(ch + NSTAGE - 1) into that stage and x_i(ch + NSTAGE - 1);
//         ds_read_b128 x 16 of chunk ch + 1 into the other register buffer
//   chain chunk ch (registers read in body ch - 1)
// Every body issues the same vector-memory ops (past the last group they read
// the next stream or the workspace slack: nothing consumes them), so the counts
// are static; the loop runs whole groups of NSTAGE chunks over the zero-filled
// streams (XC_GROUP), without a per-chunk check; the LDS reads and the register loads are inline asm
// with explicit waits (the compiler's waitcnt pass, merging across the
// rotated registers, drained vmcnt(0) every chunk).  No workgroup barrier:
// the wave is the workgroup and reads only what it staged.
// NST: the ring's stages (the loop's unroll); TWO: two chains per lane, pairs
// (i, j) and (i + 4, j) of an off-diagonal tile (ref_chain2_kernel).
// DM != 0: a dead region (DeadPlan, dead_chunk) with the dead-tap mask DM — Xc
// is the live stream, `steps` its live steps, Tc chain c's dead stream, staged
// behind each stage's J rows by NT more DMAs per chunk; a lane's pair is mixed
// when exactly one of its rows is among the nneg negated ones.
template <bool DIAG, int NST = NSTAGE, bool TWO = false, int DM = 0>
__device__ __forceinline__ void ref_chain_tile(float* lds, const Tile T, const int c, const float* __restrict__ Xc,
                                               int64_t ldc, int K, int64_t steps, int first, float* __restrict__ A,
                                               const float* __restrict__ Tc = nullptr, int nneg = 0) {
  using S = Staging<DIAG>;
  static_assert(!(TWO && DIAG), "two chains per lane on off-diagonal tiles only");
  static_assert(NST % 2 == 0 && NST >= 4, "two register buffers");
  constexpr int NT = [] {
    if constexpr (DM != 0)
      return DeadPat<DM>::NT;
    else
      return 0;
  }();
  constexpr int TCH = [] {
    if constexpr (DM != 0)
      return DeadPat<DM>::TCH;
    else
      return 0;
  }();
  static_assert(NT <= 2 && !(TWO && DM), "the dead stream's DMA statements below");
  constexpr int STG = STAGE + NT * 256;          // floats per ring stage: the J rows, then the dead stream's chunk
  constexpr int ZERO = NST * STG;                // (DM) the zero block the unmixed lanes read: NT KB
  static_assert((ZERO + NT * 256) * 4 <= NSTAGE * STAGE * 4, "inside the kernel's one LDS array");
  static_assert((NST - 1) * STG * 4 < 65536, "ds_read_b128's 16-bit offset reaches every stage");
  constexpr int NXI = TWO ? 2 : 1;               // x_i loads per body
  constexpr int OPB = S::DPW + NT + NXI;         // vector-memory ops per body
  static_assert((NST - 2) * OPB + NXI < 64, "vmcnt counts to 63");
  const int lane = threadIdx.x & 63, jl = lane & 15;
  // this lane's pair (i, j) and the staged row it reads
  const LanePair lp = lane_pair(T, lane, TWO);
  const int i = lp.i, j = lp.j, srow = lp.srow;
  const int i2 = i + IW;  // TWO: the lane's second pair (i2, j), i2 < j
  const bool valid2 = TWO && i2 < K && j < K;
  const bool valid = lp.keep && i < K && j < K;
  const int lo = i < j ? i : j, hi = i < j ? j : i;  // A holds the pair at [lo][hi]
  const int64_t rs = 8 * ldc;

  // the running sum of the previous segments: an asm load and a full wait
  // before any DMA, so no compiler-tracked load reaches into the loop
  float acc = 0.f, acc2 = 0.f;
  if (!first) {
    const float* ap = A + ((int64_t)c * K + (lo < K ? lo : K - 1)) * K + (hi < K ? hi : K - 1);
    asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(acc) : "v"(ap) : "memory");
    acc = valid ? acc : 0.f;
    if constexpr (TWO) {
      const float* ap2 = A + ((int64_t)c * K + (i2 < K ? i2 : K - 1)) * K + (j < K ? j : K - 1);
      asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(acc2) : "v"(ap2) : "memory");
      acc2 = valid2 ? acc2 : 0.f;
    }
  }

  // staging: DMA instruction u moves staged rows RPD u .. RPD u + 3, lane ->
  // row RPD u + lane / NQ, LDS slot lane % NQ holding the piece slot ^ slot_swz(row).
  // Global addresses as a uniform base (SGPRs, advanced per chunk) + a 32-bit
  // per-lane offset (the saddr form: no 64-bit address arithmetic per DMA);
  // the DMAs of a chunk share one M0 (the stage + 2 KB) and differ in the
  // instruction offset (u - 2) KB, which applies to the global and the LDS
  // address alike (13-bit signed: -2 .. +2 KB), so the lane offsets carry
  // 2 KB - (u - 2) KB of slack and the base sits 2 KB low.
  const int jrow0 = DIAG ? SB * T.X : min(SB * T.Y + JW * T.h, K - 1);  // lowest staged row (clamped)
  const char* sbj = reinterpret_cast<const char*>(Xc + (int64_t)jrow0 * rs + (int64_t)c * ldc) - 2048;
  uint32_t voj[S::DPW];
#pragma unroll
  for (int u = 0; u < S::DPW; ++u) {
    const int s = RPD * u + lane / NQ;
    int gj = DIAG ? SB * T.X + ((IW * T.g + 1 + s) & (SB - 1)) : SB * T.Y + JW * T.h + s;
    gj = gj < K ? gj : K - 1;
    voj[u] = (uint32_t)((int64_t)(gj - jrow0) * rs * 4 + 16 * ((lane % NQ) ^ slot_swz(s)) - 1024 * (u - 2) + 2048);
  }
  const uint32_t vot = 16 * lane;  // (DM) the dead stream's chunk: 16 B per lane
  // x_i: lane jl of DPP row r loads steps 4 jl .. 4 jl + 3 of the row's I row
  const int irow0 = min(SB * T.X + (TWO ? 2 * IW : IW) * T.g, K - 1);  // the wave's first I row: uniform
  const char* sbi = reinterpret_cast<const char*>(Xc + (int64_t)irow0 * rs + (int64_t)c * ldc);
  const uint32_t voi = (uint32_t)((int64_t)((i < K ? i : K - 1) - irow0) * rs * 4 + 16 * jl);
  const uint32_t voi2 = (uint32_t)((int64_t)((i2 < K ? i2 : K - 1) - irow0) * rs * 4 + 16 * jl);
  // whole loop trips of NST chunks inside the zero-filled streams (padded to
  // XC_GROUP steps, a multiple of NST * CS)
  static_assert(XC_GROUP % (NST * CS) == 0, "trips inside the zero fill");
  const int ngroup = (int)((steps + NST * CS - 1) / (NST * CS));
  // DMA(ch) into stage `slot`, then x_i(ch) into register set x (inline asm:
  // hipcc built 64-bit addresses per DMA instead of the saddr form)
  auto issue = [&](int ch, int slot, f32x4& x, f32x4& x2) {
    // the chunk's byte offset in a stream: the prefetch runs up to NSTAGE - 1
    // chunks past the last one (reads nothing consumes; the workspace carries
    // XC_SLACK bytes past the last stream)
    const int64_t co = (int64_t)ch * CS * 4;
    if (FLR_REF_ABL == 3) return;
    const char* sb = sbj + co;
    const uint32_t m = (uint32_t)(uintptr_t)lds + 4 * slot * STG + 2048;
    // M0 written in the statement that reads it; no other instruction of this
    // kernel reads M0 (the compiler emits none: checked in the ISA), so it is
    // not restored
#define FLR_DMA(n, off) "global_load_lds_dwordx4 %[v" #n "], %[sb] offset:" #off "\n\t"
    if constexpr (S::DPW == 5)
      asm volatile("s_mov_b32 m0, %[m]\n\ts_nop 0\n\t" FLR_DMA(0, -2048) FLR_DMA(1, -1024) FLR_DMA(2, 0)
                       FLR_DMA(3, 1024) FLR_DMA(4, 2048)
                   :
                   : [m] "s"(m), [sb] "s"(sb), [v0] "v"(voj[0]), [v1] "v"(voj[1]), [v2] "v"(voj[2]), [v3] "v"(voj[3]),
                     [v4] "v"(voj[S::DPW - 1])
                   : "memory");
    else
      asm volatile("s_mov_b32 m0, %[m]\n\ts_nop 0\n\t" FLR_DMA(0, -2048) FLR_DMA(1, -1024) FLR_DMA(2, 0)
                       FLR_DMA(3, 1024)
                   :
                   : [m] "s"(m), [sb] "s"(sb), [v0] "v"(voj[0]), [v1] "v"(voj[1]), [v2] "v"(voj[2]), [v3] "v"(voj[3])
                   : "memory");
#undef FLR_DMA
    static_assert(S::DPW == 4 || S::DPW == 5, "the DMA statements above");
    if constexpr (NT > 0) {  // the dead stream's chunk: lane l's 16 B at byte 16 l of the stage's T area
      const char* st = reinterpret_cast<const char*>(Tc) + (int64_t)ch * TCH * 4;
      const uint32_t mt = (uint32_t)(uintptr_t)lds + 4 * (slot * STG + STAGE);
      if constexpr (NT == 2)
        asm volatile("s_mov_b32 m0, %[m]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v], %[sb] offset:0\n\t"
                     "global_load_lds_dwordx4 %[v], %[sb] offset:1024"
                     :
                     : [m] "s"(mt), [sb] "s"(st), [v] "v"(vot)
                     : "memory");
      else
        asm volatile("s_mov_b32 m0, %[m]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[v], %[sb] offset:0"
                     :
                     : [m] "s"(mt), [sb] "s"(st), [v] "v"(vot)
                     : "memory");
    }
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x) : "v"(voi), "s"(sbi + co) : "memory");
    if constexpr (TWO) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x2) : "v"(voi2), "s"(sbi + co) : "memory");
  };
  // per-lane LDS byte addresses of staged row srow's 16 swizzled pieces in stage 0
  const int rsw = slot_swz(srow);
  uint32_t ra[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) ra[q] = (uint32_t)(uintptr_t)(lds + srow * CS + 4 * (q ^ rsw));
  auto rows = [](auto st, f32x4(&v)[NQ], const uint32_t(&a)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (FLR_REF_ABL != 2)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v[q]) : "v"(a[q]), "n"(decltype(st)::value * STG * 4)
                     : "memory");
  };

  // (DM) the dead stream's LDS address per stage: the stage's T area on a mixed
  // lane, the zero block (zeroed here, by this wave) on the others
  uint32_t ta[NST];
  if constexpr (DM != 0) {
    const bool mixed = valid && ((i < nneg) != (j < nneg));
    static_assert(NT * 256 % 64 == 0, "the zero block in whole 16-B pieces per lane");
#pragma unroll
    for (int q = 0; q < NT * 256 / 256; ++q)
      *reinterpret_cast<f32x4*>(lds + ZERO + 256 * q + 4 * lane) = f32x4{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < NST; ++u)
      ta[u] = (uint32_t)(uintptr_t)(mixed ? lds + u * STG + STAGE : lds + ZERO);
  }
  f32x4 va[NQ], vb[NQ];
  f32x4 xs[NST], xs2[NST];
  auto body = [&](auto U, int ch, f32x4(&vc)[NQ], f32x4(&vn)[NQ]) {
    constexpr int u = decltype(U)::value;
    // DMA(ch + 1) was issued in body ch + 2 - NSTAGE; younger than it: its
    // x_i load and the NSTAGE - 3 bodies since (x_i(ch) is older: covered)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 3) * OPB + NXI) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // chunk ch's x_j
    // chunk ch's operands arrived at the waits above: tie them to here
    asm volatile("" : "+v"(vc[0]), "+v"(vc[1]), "+v"(vc[2]), "+v"(vc[3]), "+v"(vc[4]), "+v"(vc[5]), "+v"(vc[6]),
                 "+v"(vc[7]), "+v"(vc[8]), "+v"(vc[9]), "+v"(vc[10]), "+v"(vc[11]), "+v"(vc[12]), "+v"(vc[13]),
                 "+v"(vc[14]), "+v"(vc[15]), "+v"(xs[u]));
    if constexpr (TWO) asm volatile("" : "+v"(xs2[u]));
    issue(ch + NST - 1, (u + NST - 1) % NST, xs[(u + NST - 1) % NST], xs2[(u + NST - 1) % NST]);
    rows(std::integral_constant<int, (u + 1) % NST>{}, vn, ra);
    if constexpr (DM != 0)
      acc = dead_chunk<DM>(xs[u], vc, acc, ta[u]);
    else if constexpr (TWO)
      chain_chunk2(xs[u], xs2[u], vc, acc, acc2);
    else if (FLR_REF_ABL != 5)
      acc = chain_chunk(xs[u], vc, acc);
  };
  // prologue = the issues of bodies -(NSTAGE-1) .. -1, then chunk 0's rows
#pragma unroll
  for (int u = 0; u < NST - 1; ++u) issue(u, u, xs[u], xs2[u]);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * OPB + NXI) : "memory");  // DMA(0)
  rows(std::integral_constant<int, 0>{}, va, ra);
  for (int ch = 0; ch < ngroup * NST; ch += NST)
    static_for(
        [&](auto U) {
          constexpr int u = decltype(U)::value;
          if constexpr (u % 2 == 0)
            body(U, ch + u, va, vb);
          else
            body(U, ch + u, vb, va);
        },
        std::make_integer_sequence<int, NST>{});
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (valid) A[((int64_t)c * K + lo) * K + hi] = acc;
  if (valid2) A[((int64_t)c * K + i2) * K + j] = acc2;
}

// grid 8 x (t1 - t0) one-wave workgroups: chain c = blockIdx % 8 (the XCD),
// tile t0 + blockIdx / 8
__global__ __launch_bounds__(64) void ref_chain_kernel(const float* __restrict__ Xc, int64_t ldc, int K,
                                                       int64_t steps, int t0, int first, float* __restrict__ A) {
  // ONE __shared__ array (a second __shared__ object makes hipcc wait vmcnt(0)
  // before the LDS reads, draining the DMA ring)
  __shared__ __attribute__((aligned(16))) float lds[NSTAGE * STAGE];
  const int c = (int)(blockIdx.x & 7);
  const Tile T = tile_of(t0 + (int)(blockIdx.x >> 3));
  if (T.diag)
    ref_chain_tile<true>(lds, T, c, Xc, ldc, K, steps, first, A);
  else
    ref_chain_tile<false>(lds, T, c, Xc, ldc, K, steps, first, A);
}

// A dead region (DeadPlan) of every tile: grid as ref_chain_kernel, t0 = 0.
// A same-kind pair's dead steps are fma(+0, +0, s) = s (fl(g - g) = +0 for
// finite g; ref_finish_kernel covers the rest), so a wave without a mixed pair
// runs the live stream alone, through the plain tile; a wave with one runs the
// two streams in the chain's order.  Same LDS array as ref_chain_kernel: four
// workgroups per CU.
template <int DM>
__global__ __launch_bounds__(64) void ref_chain_dead_kernel(const float* __restrict__ Xl, int64_t ldc,
                                                            const float* __restrict__ Tb, int64_t ldt, int K,
                                                            int nneg, int64_t steps, int first,
                                                            float* __restrict__ A) {
  __shared__ __attribute__((aligned(16))) float lds[NSTAGE * STAGE];
  const int c = (int)(blockIdx.x & 7);
  const Tile T = tile_of((int)(blockIdx.x >> 3));
  // the lane's pair, as ref_chain_tile numbers them
  const LanePair lp = lane_pair(T, (int)(threadIdx.x & 63), false);
  const bool mixed = lp.keep && lp.i < K && lp.j < K && ((lp.i < nneg) != (lp.j < nneg));
  const float* Tc = Tb + (int64_t)c * ldt;
  if (__builtin_amdgcn_ballot_w64(mixed) == 0) {
    if (T.diag)
      ref_chain_tile<true>(lds, T, c, Xl, ldc, K, steps, first, A);
    else
      ref_chain_tile<false>(lds, T, c, Xl, ldc, K, steps, first, A);
  } else if (T.diag) {
    ref_chain_tile<true, NSTD, false, DM>(lds, T, c, Xl, ldc, K, steps, first, A, Tc, nneg);
  } else {
    ref_chain_tile<false, NSTD, false, DM>(lds, T, c, Xl, ldc, K, steps, first, A, Tc, nneg);
  }
}

// K >= 256 (more tiles than SIMDs: the chains are throughput-bound, not
// latency-bound): off-diagonal super-block pairs as 8 waves of 8 I rows x 16 J
// rows, two chains per lane sharing the staged x_j (half the LDS reads per chain
// step), diagonal super-blocks as the 1-I circulant tiles above; a 4-stage ring
// (20 KB) and at most 256 VGPRs, so two waves per SIMD.  Tiles per Y: the
// off-diagonal pairs X = 0 .. Y-1 (8 waves each: w = 2g + h), then the diagonal.
constexpr int NST2 = 4;
__global__ __launch_bounds__(64, 2) void ref_chain2_kernel(const float* __restrict__ Xc, int64_t ldc, int K,
                                                           int64_t steps, int first, float* __restrict__ A) {
  __shared__ __attribute__((aligned(16))) float lds[NST2 * STAGE];
  const int c = (int)(blockIdx.x & 7);
  const Tile T = tile2_of((int)(blockIdx.x >> 3));
  if (T.diag)
    ref_chain_tile<true, NST2, false>(lds, T, c, Xc, ldc, K, steps, first, A);
  else
    ref_chain_tile<false, NST2, true>(lds, T, c, Xc, ldc, K, steps, first, A);
}

int launch_ref_chain(const float* Xc, int64_t ldc, int64_t K, int64_t steps, int t0, int t1, int first, float* A,
                     hipStream_t st) {
  hipLaunchKernelGGL(ref_chain_kernel, dim3(8 * (t1 - t0)), dim3(64), 0, st, Xc, ldc, (int)K, steps, t0, first, A);
  return launch_status("ref_chain_kernel");
}

int launch_ref_chain2(const float* Xc, int64_t ldc, int64_t K, int64_t steps, int first, float* A, hipStream_t st) {
  hipLaunchKernelGGL(ref_chain2_kernel, dim3(8 * ntiles2_of((int)K)), dim3(64), 0, st, Xc, ldc, (int)K, steps, first,
                     A);
  return launch_status("ref_chain2_kernel");
}

int launch_ref_chain_dead(int dm, const float* Xl, int64_t ldc, const float* Tb, int64_t ldt, int64_t K, int nneg,
                          int64_t steps, int first, float* A, hipStream_t st) {
  auto kern = dm == DM_ONE ? ref_chain_dead_kernel<DM_ONE> : ref_chain_dead_kernel<DM_FOUR>;
  hipLaunchKernelGGL(kern, dim3(8 * ntiles_of((int)K)), dim3(64), 0, st, Xl, ldc, Tb, ldt, (int)K, nneg, steps, first,
                     A);
  return launch_status("ref_chain_dead_kernel");
}

}  // namespace pwref
}  // namespace flr
