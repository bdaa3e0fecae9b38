// Tap-major GEMM engine, unit 3 of 5: the data gradient (DgradT, one launch
// per stride-parity class).
#include "conv_t_kernels.h"

using namespace flr;

extern "C" int flr_conv2d_bwd_data_t(const float* dy, const float* w_t, float* dx, int64_t K, int64_t B, int64_t Cin,
                                     int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                     int64_t pad, void* ws, size_t ws_bytes, void* stream) {
  return flr_conv2d_bwd_data_t_add(dy, w_t, nullptr, dx, K, B, Cin, H, W, Cout, KH, KW, stride, pad, ws, ws_bytes,
                                   stream);
}

extern "C" int flr_conv2d_bwd_data_t_add(const float* dy, const float* w_t, const float* add, float* dx, int64_t K,
                                         int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH,
                                         int64_t KW, int64_t stride, int64_t pad, void* ws, size_t ws_bytes,
                                         void* stream) {
  return flr_conv2d_bwd_data_t_ex(dy, w_t, KH * KW * Cin * Cout, add, dx, K, B, Cin, H, W, Cout, KH, KW, stride, pad,
                                  ws, ws_bytes, stream);
}

extern "C" int flr_conv2d_bwd_data_t_ex(const float* dy, const float* w_t, int64_t w_stride, const float* add,
                                        float* dx, int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                        int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad, void* ws,
                                        size_t ws_bytes, void* stream) {
  if (!dy || !w_t || !dx || w_stride < 0) return FLR_ERR_ARG;
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad))
    return conv::geom_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad) ? FLR_ERR_UNSUPPORTED : FLR_ERR_ARG;
  if (stride > 4) return FLR_ERR_UNSUPPORTED;  // <= MAX_CLASSES parity classes
  const conv::Geom g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  convt::DgradT cls[convt::MAX_CLASSES];
  const int nc = convt::dgrad_classes(g, cls);
  for (int c = 0; c < nc; ++c) {
    // in-place accumulation (add == dx): a class no tap reaches adds nothing
    if (add == dx && cls[c].R() == 0) continue;
    cls[c].dy = dy; cls[c].w = w_t; cls[c].dx = dx; cls[c].add = add; cls[c].wsk = w_stride;
    const int rc = convt::launch(cls[c], ws, ws_bytes, as_stream(stream), "conv bwd data (tap-major)");
    if (rc != FLR_OK) return rc;
  }
  return FLR_OK;
}
