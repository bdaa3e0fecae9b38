// Tap-major GEMM engine, unit 2 of 5: the convolution forward (FwdT).
#include "conv_t_launch.h"

using namespace flr;

extern "C" int flr_conv2d_fwd_t(const float* x, const float* w_t, float* y, int64_t K, int64_t B, int64_t Cin,
                                int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                int64_t pad, void* ws, size_t ws_bytes, void* stream) {
  return flr_conv2d_fwd_t_ex(x, w_t, KH * KW * Cin * Cout, y, K, B, Cin, H, W, Cout, KH, KW, stride, pad, ws,
                             ws_bytes, stream);
}

extern "C" int flr_conv2d_resident_ok(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                      int64_t KH, int64_t KW, int64_t stride, int64_t pad, int dgrad) {
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad)) return 0;
  const conv::Geom g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  if (!dgrad) {
    convt::FwdT pl;
    pl.g = g;
    pl.x = pl.w = nullptr; pl.y = nullptr; pl.wsk = 0;
    return convt::resident_ok(pl) ? 1 : 0;
  }
  convt::DgradT cls[convt::MAX_CLASSES];
  const int nc = convt::dgrad_classes(g, cls);
  return nc == 1 && convt::resident_ok(cls[0]) ? 1 : 0;
}

extern "C" int flr_conv2d_fwd_t_ex(const float* x, const float* w_t, int64_t w_stride, float* y, int64_t K, int64_t B,
                                   int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                                   int64_t stride, int64_t pad, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !w_t || !y || w_stride < 0) return FLR_ERR_ARG;
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad))
    return conv::geom_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad) ? FLR_ERR_UNSUPPORTED : FLR_ERR_ARG;
  convt::FwdT pl;
  pl.g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  pl.x = x; pl.w = w_t; pl.y = y; pl.wsk = w_stride;
  return convt::launch(pl, ws, ws_bytes, as_stream(stream), "conv fwd (tap-major)");
}
