// Tap-major GEMM engine, unit 4 of 5: the weight gradient (WgtT) with its
// clip-norm partials, the dead-tap zero fill and the resident form's probe.
#include "conv_t_launch.h"

namespace flr {
namespace convt {
// dw_t slabs [k][t] of the taps set in `dead` = 0 (grid: 64 x K).
__global__ void zero_taps_kernel(float* __restrict__ dw, int KK, int64_t slab, uint64_t dead) {
  const int k = blockIdx.y;
  for (int t = 0; t < KK; ++t) {
    if (!((dead >> t) & 1)) continue;
    f32x4* p = reinterpret_cast<f32x4*>(dw + ((int64_t)k * KK + t) * slab);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slab / 4; i += (int64_t)gridDim.x * blockDim.x)
      p[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
}  // namespace convt
}  // namespace flr

using namespace flr;

extern "C" int flr_conv2d_bwd_weight_t(const float* x, const float* dy, float* dw_t, int64_t K, int64_t B,
                                       int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                                       int64_t stride, int64_t pad, int zero_dead_taps, void* ws, size_t ws_bytes,
                                       void* stream) {
  return flr_conv2d_bwd_weight_t_sq(x, dy, dw_t, K, B, Cin, H, W, Cout, KH, KW, stride, pad, zero_dead_taps, nullptr,
                                    0, ws, ws_bytes, stream);
}

extern "C" int64_t flr_conv2d_bwd_weight_t_sq_slots(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                                    int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                                    int64_t pad) {
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad)) return -1;
  convt::WgtT<true> pl;  // the slot count does not depend on the B-operand load form
  pl.g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  return convt::sq_slots(pl);
}

extern "C" int flr_conv2d_wgrad_resident_ok(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                            int64_t KH, int64_t KW, int64_t stride, int64_t pad) {
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad)) return 0;
  const conv::Geom g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  if ((g.Ho * g.Wo) % 4 != 0) return 0;  // WgtT<false>
  convt::WgtT<true> pl;
  pl.g = g;
  pl.x = pl.dy = nullptr; pl.dw = nullptr;
  return convt::wgrad_resident_ok(pl) ? 1 : 0;
}

extern "C" int flr_conv2d_bwd_weight_t_sq(const float* x, const float* dy, float* dw_t, int64_t K, int64_t B,
                                          int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                                          int64_t stride, int64_t pad, int zero_dead_taps, double* sq,
                                          int64_t sq_ld, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw_t) return FLR_ERR_ARG;
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad))
    return conv::geom_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad) ? FLR_ERR_UNSUPPORTED : FLR_ERR_ARG;
  const conv::Geom g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  hipStream_t st = as_stream(stream);
  if (zero_dead_taps && g.ntaps < KH * KW) {  // dead taps: exact-zero gradients, one slab each
    uint64_t dead = (KH * KW >= 64) ? ~0ull : ((1ull << (KH * KW)) - 1);
    for (int t = 0; t < g.ntaps; ++t) dead &= ~(1ull << (g.tap_kh[t] * KW + g.tap_kw[t]));
    hipLaunchKernelGGL(convt::zero_taps_kernel, dim3(64, (unsigned)K), dim3(256), 0, st, dw_t, (int)(KH * KW),
                       (int64_t)Cin * Cout, dead);
    const int rc = launch_status("conv bwd weight: zero dead taps");
    if (rc != FLR_OK) return rc;
  }
  if (sq) {  // the partial slots follow the launch's split choice, which needs the full workspace
    convt::WgtT<true> probe;
    probe.g = g;
    if (sq_ld < convt::sq_slots(probe) || ws_bytes < convt::splits_bytes(probe) ||
        (convt::splits_bytes(probe) > 0 && !ws))
      return FLR_ERR_WORKSPACE;
  }
  if ((g.Ho * g.Wo) % 4 == 0) {
    convt::WgtT<true> pl;
    pl.g = g; pl.x = x; pl.dy = dy; pl.dw = dw_t; pl.sq = sq; pl.sq_ld = (int)sq_ld;
    return convt::launch(pl, ws, ws_bytes, st, "conv bwd weight (tap-major)");
  }
  convt::WgtT<false> pl;
  pl.g = g; pl.x = x; pl.dy = dy; pl.dw = dw_t; pl.sq = sq; pl.sq_ld = (int)sq_ld;
  return convt::launch(pl, ws, ws_bytes, st, "conv bwd weight (tap-major)");
}
