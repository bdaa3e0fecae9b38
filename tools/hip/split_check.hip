// Bit-compares the two shipped forms of the bf16x3 split (csrc/bf16x6.h; round-
// to-nearest hi, mid, lo): split3_sub, bf16 -> fp32 expansion + subtraction (the
// GRU, the stem), and split3_dot2, the v_dot2_f32_bf16 residual (the conv
// engine).  Random fp32 bit patterns over every finite exponent, plus signed
// zeros and denormals.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/hip/split_check.hip -o tools/hip/split_check
#include "../../multimodal-fl-security_amd/csrc/bf16x6.h"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

// one thread: 8 consecutive values, the unit both forms take
__global__ void split_both(const float* __restrict__ x, int n, unsigned* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (8 * i + 7 >= n) return;
  float v[8];
  for (int e = 0; e < 8; ++e) v[e] = x[8 * i + e];
  flr::bf16x8 sh, sm, sl, dh, dm, dl;
  flr::split3_sub(v, sh, sm, sl);
  flr::split3_dot2(v, dh, dm, dl);
  auto u = [](__bf16 z) { return (unsigned)__builtin_bit_cast(unsigned short, z); };
  // a mismatch is an error unless the value's residual is denormal (|v| < 2^-100),
  // its bf16 rounding overflows (|v| > 0x1.fep127, where both forms give inf/nan), or
  // the rounding of its dot2 pair partner does (element e ^ 1, the other half of the
  // same v_dot2 operand): there inf * 0 makes the dot2 residual NaN while the
  // subtraction form stays finite (bf16x6.h).  The count without the last exemption
  // is printed too.
  auto plain = [](float f) { return fabsf(f) >= 0x1p-100f && fabsf(f) <= 0x1.fep127f; };
  for (int e = 0; e < 8; ++e) {
    const unsigned m = (u(sh[e]) != u(dh[e])) | ((u(sm[e]) != u(dm[e])) << 1) | ((u(sl[e]) != u(dl[e])) << 2);
    if (!m) continue;
    atomicOr(bad, m);
    const unsigned slot = atomicAdd(bad + 1, 1u);
    if (slot < 16) bad[2 + slot] = __builtin_bit_cast(unsigned, v[e]);  // the first mismatching values
    if (plain(v[e])) atomicAdd(bad + 18, 1u);
    if (plain(v[e]) && fabsf(v[e ^ 1]) <= 0x1.fep127f) atomicAdd(bad + 19, 1u);
  }
}

int main() {
  const int n = 1 << 24;
  std::vector<float> h(n);
  std::mt19937 g(7);
  for (int i = 0; i < n; ++i) {
    uint32_t b = g();
    if ((b & 0x7f800000u) == 0x7f800000u) b &= ~0x40000000u;  // no inf/nan
    if (i % 97 == 0) b &= 0x807fffffu;                        // denormals and signed zeros
    h[i] = __builtin_bit_cast(float, b);
  }
  float* d;
  unsigned* bad;
  if (hipMalloc(&d, n * 4) || hipMalloc(&bad, 20 * 4)) return 2;
  if (hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice) || hipMemset(bad, 0, 20 * 4)) return 2;
  split_both<<<(n / 8 + 255) / 256, 256>>>(d, n, bad);
  unsigned r[20];
  if (hipMemcpy(r, bad, 20 * 4, hipMemcpyDeviceToHost)) return 2;
  printf("split_check: %d values, split3_sub vs split3_dot2: mismatch mask %u, mismatching values %u, outside the "
         "denormal / own-overflow ranges %u, of those with a pair partner that does not overflow (errors) %u\n",
         n, r[0], r[1], r[18], r[19]);
  for (unsigned i = 0; i < 16 && i < r[1]; ++i) printf("  value %g\n", __builtin_bit_cast(float, r[2 + i]));
  return r[19] ? 1 : 0;
}
