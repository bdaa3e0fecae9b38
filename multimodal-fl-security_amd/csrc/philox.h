// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as
// 1, 2, 3", SC 2011), written out: no RNG library is linked.  The counter-based
// generator of attack_fang.hip (flr_fang_trim_rows: word 0 per draw) and
// agg_flame.hip (flr_add_gaussian: the four words of a block); flr.h writes the
// round out.  Integer arithmetic only: the same bits in every caller.
#pragma once

#include "flr_common.h"

namespace flr {

// The four words of counter (c0, c1, c2, c3) under key (k0, k1), in place.
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
}

// Word 0 alone.
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
  philox4x32_10(c0, c1, c2, c3, k0, k1);
  return c0;
}

}  // namespace flr
