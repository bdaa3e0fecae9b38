// The bf16x6 form of an fp32 product, shared by every GEMM on the training path
// (the tap-major conv engine, the stem, the GRU recurrence): raw buffer loads,
// the split of an fp32 operand into three bf16 terms, and the ONE order in which
// the six bf16 products of a 16-deep k-step enter an accumulator.
//
// f32 MFMA runs at 1/16 of the bf16 rate on gfx950.  Each f32 operand is split
// into three round-to-nearest bf16 terms, x = hi + mid + lo (the residual is
// below 2^-24 |x|: 24 significand bits in three 8-bit pieces), and the six
// products whose order is above 2^-24 (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo,
// lo*hi; every bf16 x bf16 product is exact in the fp32 accumulator) run on
// v_mfma_f32_32x32x16_bf16: 6 x 32 cycles per 16-deep k-step against 8 x 64 for
// v_mfma_f32_32x32x2_f32, at a per-product error of a few 2^-24 |a b| — the
// rounding of an fp32 product.  Lane (l32, h) supplies row l32 and reduction
// indices k0 .. k0+7, k0 = 16 s + 8 h.
#pragma once

#include "flr_common.h"

namespace flr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Raw buffer loads: an out-of-range byte offset returns 0 with no branch, so a
// wave's loads stay in flight together and a padding element costs no VALU work.
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr unsigned SENT = 0x80000000u;  // out-of-range voffset (every buffer is < 2 GB): the load returns 0

__device__ __forceinline__ rsrc_t make_rsrc(const float* p, int64_t nfloats) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int bytes = __builtin_amdgcn_readfirstlane((int)(nfloats * 4));
  void* b = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(b, (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ float ld1(rsrc_t r, unsigned voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 ld4(rsrc_t r, unsigned voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// ---- the split: term 0 = hi, 1 = mid, 2 = lo ----------------------------------
// Two forms with the same bits and different instructions; a caller keeps the one
// it was measured with.  tools/hip/split_check.hip compares them on 2^24 patterns:
// they agree except where a value's bf16 rounding overflows (|v| > 0x1.fep127), and
// there split3_dot2 also turns the mid / lo terms of the value it is paired with
// (elements 2p, 2p + 1 share a v_dot2 operand: inf * 0) into NaN.
//
// split3_sub: bf16 -> fp32 expansion and a subtraction per residual (the GRU, the stem).
__device__ __forceinline__ void split1_sub(float v, __bf16& hi, __bf16& mid, __bf16& lo) {
  hi = (__bf16)v;
  const float r1 = v - (float)hi;
  mid = (__bf16)r1;
  lo = (__bf16)(r1 - (float)mid);
}
__device__ __forceinline__ void split3_sub(const float (&v)[8], bf16x8& hi, bf16x8& mid, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 a, b, c;
    split1_sub(v[j], a, b, c);
    hi[j] = a;
    mid[j] = b;
    lo[j] = c;
  }
}
// split3_dot2 (the conv engine): the residuals r = v - (float)bf16(v) come from
// v_dot2_f32_bf16 against (-1, 0) / (0, -1): one instruction per value instead of
// the expansion plus the subtraction.  r is exact either way (|r| <= half a bf16
// ulp of v, representable in fp32), so the terms are split3_sub's.
__device__ __forceinline__ void split3_dot2(const float (&v)[8], bf16x8& hi, bf16x8& mid, bf16x8& lo) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  // (-1, 0) and (0, -1) as opaque SGPRs: hipcc encodes a (-1, 0) constant as the
  // inline constant -1.0, which the hardware reads as the fp32 bits, i.e. (0, -1)
  unsigned klo, khi;  // non-volatile: the compiler may hoist / share them
  asm("s_mov_b32 %0, 0xbf80" : "=s"(klo));
  asm("s_mov_b32 %0, 0xbf800000" : "=s"(khi));
  const bf16x2 nl = __builtin_bit_cast(bf16x2, klo), nh = __builtin_bit_cast(bf16x2, khi);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float v0 = v[2 * p], v1 = v[2 * p + 1];
    const bf16x2 a = {(__bf16)v0, (__bf16)v1};
    const float r0 = __builtin_amdgcn_fdot2_f32_bf16(a, nl, v0, false);
    const float r1 = __builtin_amdgcn_fdot2_f32_bf16(a, nh, v1, false);
    const bf16x2 b = {(__bf16)r0, (__bf16)r1};
    const float s0 = __builtin_amdgcn_fdot2_f32_bf16(b, nl, r0, false);
    const float s1 = __builtin_amdgcn_fdot2_f32_bf16(b, nh, r1, false);
    hi[2 * p] = a[0];
    hi[2 * p + 1] = a[1];
    mid[2 * p] = b[0];
    mid[2 * p + 1] = b[1];
    lo[2 * p] = (__bf16)s0;
    lo[2 * p + 1] = (__bf16)s1;
  }
}

// ---- the product order ---------------------------------------------------------
// (term of A, term of B) of the six products of a k-step, small terms first:
// mid*mid, hi*lo, lo*hi, hi*mid, mid*hi, hi*hi.  Bit-identical models at any GPU
// count and every "equals the form it replaces" guarantee rest on each kernel
// form taking this order from here.
constexpr int X6_ORDER[6][2] = {{1, 1}, {0, 2}, {2, 0}, {0, 1}, {1, 0}, {0, 0}};

// product P of the order into one accumulator, the terms given one by one (a kernel that keeps
// one array per term calls this per block: tgemm_kernel)
template <int T>
__device__ __forceinline__ const bf16x8& x6_term(const bf16x8& hi, const bf16x8& mid, const bf16x8& lo) {
  return T == 0 ? hi : T == 1 ? mid : lo;
}
template <int P>
__device__ __forceinline__ void mfma6_product(f32x16& c, const bf16x8& ah, const bf16x8& am, const bf16x8& al,
                                              const bf16x8& bh, const bf16x8& bm, const bf16x8& bl) {
  constexpr int TA = X6_ORDER[P][0], TB = X6_ORDER[P][1];
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x6_term<TA>(ah, am, al), x6_term<TB>(bh, bm, bl), c, 0, 0, 0);
}

// The chain of one accumulator: c + the six products.  Terms one by one, or a[3] x b[3].
__device__ __forceinline__ f32x16 mfma6(f32x16 c, const bf16x8& ah, const bf16x8& am, const bf16x8& al,
                                        const bf16x8& bh, const bf16x8& bm, const bf16x8& bl) {
  mfma6_product<0>(c, ah, am, al, bh, bm, bl);
  mfma6_product<1>(c, ah, am, al, bh, bm, bl);
  mfma6_product<2>(c, ah, am, al, bh, bm, bl);
  mfma6_product<3>(c, ah, am, al, bh, bm, bl);
  mfma6_product<4>(c, ah, am, al, bh, bm, bl);
  mfma6_product<5>(c, ah, am, al, bh, bm, bl);
  return c;
}
__device__ __forceinline__ f32x16 mfma6(f32x16 c, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  return mfma6(c, a[0], a[1], a[2], b[0], b[1], b[2]);
}

// Product-major over a wave's MI x NJ accumulator blocks: the blocks' chains
// interleave, so a chain's next MFMA never waits on its own previous one.  Per
// accumulator the order is mfma6's.  The terms of block row i / column j are
// fa[i][3] / fb[j][3].
template <int P, int MI, int NJ>
__device__ __forceinline__ void mfma6_product_blocks(f32x16 (&acc)[MI][NJ], const bf16x8 (&fa)[MI][3],
                                                     const bf16x8 (&fb)[NJ][3]) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      mfma6_product<P>(acc[i][j], fa[i][0], fa[i][1], fa[i][2], fb[j][0], fb[j][1], fb[j][2]);
}
template <int MI, int NJ>
__device__ __forceinline__ void mfma6_blocks(f32x16 (&acc)[MI][NJ], const bf16x8 (&fa)[MI][3],
                                             const bf16x8 (&fb)[NJ][3]) {
  mfma6_product_blocks<0>(acc, fa, fb);
  mfma6_product_blocks<1>(acc, fa, fb);
  mfma6_product_blocks<2>(acc, fa, fb);
  mfma6_product_blocks<3>(acc, fa, fb);
  mfma6_product_blocks<4>(acc, fa, fb);
  mfma6_product_blocks<5>(acc, fa, fb);
}

}  // namespace flr
