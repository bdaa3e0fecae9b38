// Tap-major GEMM engine, unit 3 of 5: the data gradient (DgradT, one launch
// per stride-parity class, or the fused stride-2 form of conv_t_dgrad_fused.h).
#include "conv_t_dgrad_fused.h"

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
  return flr_conv2d_bwd_data_t_sc(dy, w_t, w_stride, add, dx, K, B, Cin, H, W, Cout, KH, KW, stride, pad, nullptr,
                                  nullptr, 0, 0, ws, ws_bytes, stream);
}

namespace {
// the classes of one conv with its operands set; the status of the argument checks
int dgrad_plan(const float* dy, const float* w_t, int64_t w_stride, const float* add, float* dx, int64_t K, int64_t B,
               int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
               conv::Geom& g, convt::DgradT* cls, int& nc) {
  if (!dy || !w_t || !dx || w_stride < 0) return FLR_ERR_ARG;
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad))
    return conv::geom_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad) ? FLR_ERR_UNSUPPORTED : FLR_ERR_ARG;
  if (stride > 4) return FLR_ERR_UNSUPPORTED;  // <= MAX_CLASSES parity classes
  g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  nc = convt::dgrad_classes(g, cls);
  for (int c = 0; c < nc; ++c) {
    cls[c].dy = dy; cls[c].w = w_t; cls[c].dx = dx; cls[c].add = add; cls[c].wsk = w_stride;
  }
  return FLR_OK;
}

int dgrad_per_class(const convt::DgradT* cls, int nc, void* ws, size_t ws_bytes, void* stream) {
  for (int c = 0; c < nc; ++c) {
    // in-place accumulation (add == dx): a class no tap reaches adds nothing
    if (cls[c].add == cls[c].dx && cls[c].R() == 0) continue;
    const int rc = convt::launch(cls[c], ws, ws_bytes, as_stream(stream), "conv bwd data (tap-major)");
    if (rc != FLR_OK) return rc;
  }
  return FLR_OK;
}
}  // namespace

extern "C" int flr_conv2d_bwd_data_t_sc(const float* dy, const float* w_t, int64_t w_stride, const float* add,
                                        float* dx, int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                        int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                                        const float* dy_ds, const float* w_ds, int64_t w_ds_stride, int64_t Cout_ds,
                                        void* ws, size_t ws_bytes, void* stream) {
  conv::Geom g, gs;
  convt::DgradT cls[convt::MAX_CLASSES], scls[convt::MAX_CLASSES];
  int nc = 0, nsc = 0;
  int rc = dgrad_plan(dy, w_t, w_stride, add, dx, K, B, Cin, H, W, Cout, KH, KW, stride, pad, g, cls, nc);
  if (rc != FLR_OK) return rc;
  const bool sc = dy_ds || w_ds;
  if (sc) {  // the block's 1x1 shortcut at the same stride, accumulated onto dx
    rc = dgrad_plan(dy_ds, w_ds, w_ds_stride, dx, dx, K, B, Cin, H, W, Cout_ds, 1, 1, stride, 0, gs, scls, nsc);
    if (rc != FLR_OK) return rc;
  }
  if (convt::dgrad_fused_ok(g, cls, nc, add, dx, sc ? &gs : nullptr)) {
    convt::DgradFusedArgs fa;
    for (int c = 0; c < convt::FD_CLASSES; ++c) {
      fa.cls[c] = cls[c];
      fa.S[c] = convt::resolve(cls[c], ws, ws_bytes).S;
    }
    fa.sc = sc ? scls[0] : cls[0];
    fa.Ssc = sc ? convt::resolve(scls[0], ws, ws_bytes).S : 0;
    return convt::launch_dgrad_fused(fa, as_stream(stream), "conv bwd data (tap-major, fused classes)");
  }
  rc = dgrad_per_class(cls, nc, ws, ws_bytes, stream);
  if (rc != FLR_OK || !sc) return rc;
  return dgrad_per_class(scls, nsc, ws, ws_bytes, stream);
}

// the geometry's classes, for the queries below (0 classes: not a tap-major data gradient)
static int query_classes(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                         int64_t stride, int64_t pad, conv::Geom& g, convt::DgradT* cls) {
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad) || stride > 4) return 0;
  g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  return convt::dgrad_classes(g, cls);
}

extern "C" int flr_conv2d_dgrad_fused_supported(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                                int64_t KH, int64_t KW, int64_t stride, int64_t pad) {
  conv::Geom g;
  convt::DgradT cls[convt::MAX_CLASSES];
  const int nc = query_classes(K, B, Cin, H, W, Cout, KH, KW, stride, pad, g, cls);
  return nc == convt::FD_CLASSES && convt::dgrad_fused_geom_ok(g) ? 1 : 0;
}

extern "C" int flr_conv2d_dgrad_fused_preferred(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                                int64_t KH, int64_t KW, int64_t stride, int64_t pad, int shortcut) {
  conv::Geom g;
  convt::DgradT cls[convt::MAX_CLASSES];
  const int nc = query_classes(K, B, Cin, H, W, Cout, KH, KW, stride, pad, g, cls);
  if (nc != convt::FD_CLASSES || !convt::dgrad_fused_geom_ok(g)) return 0;
  const int kn = convt::dgrad_fused_knob();
  return kn >= 0 ? kn : (convt::dgrad_fused_preferred(g, shortcut != 0) ? 1 : 0);
}

extern "C" int flr_conv2d_dgrad_class_splits(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                             int64_t KH, int64_t KW, int64_t stride, int64_t pad, int cls_index,
                                             size_t ws_bytes) {
  conv::Geom g;
  convt::DgradT cls[convt::MAX_CLASSES];
  const int nc = query_classes(K, B, Cin, H, W, Cout, KH, KW, stride, pad, g, cls);
  if (cls_index < 0 || cls_index >= nc) return 0;
  // any non-null workspace pointer: only its size enters the choice
  return convt::resolve(cls[cls_index], ws_bytes ? &g : nullptr, ws_bytes).S;
}
