// Tap-major GEMM engine, unit 1 of 5: the explicit / gathered im2col path of
// the short-reduction convolutions (the stem; Dense* and Stem* plans) and the
// tap-major workspace query.
#include "conv_t_launch.h"

namespace flr {
namespace convt {

// col[k][pix][RP] (grid: pixel blocks x K).  A workgroup builds IM_PB whole
// rows in LDS — one thread per (pix, ci, kh) fills the KW-long run
// r = (ci*KH + kh)*KW + 0..KW-1 — then streams the IM_PB*RP contiguous floats
// out as 16-B stores (RP % 4 == 0).
constexpr int IM_PB = 32, IM_MAXRP = 512;
__global__ __launch_bounds__(THREADS) void im2col_kernel(const Geom g, const float* __restrict__ x, int RP,
                                                         float* __restrict__ col) {
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [IM_PB][RP]
  const int k = blockIdx.y;
  const int N = g.B * g.Ho * g.Wo, CK = g.Cin * g.KH, R = CK * g.KW;
  const int pix0 = blockIdx.x * IM_PB;
  const int np = min(IM_PB, N - pix0);
  const float* xk = x + k * g.sxk;
  for (int e = threadIdx.x; e < np * CK; e += THREADS) {
    const int pl = e / CK, j = e - pl * CK;
    const int ci = j / g.KH, kh = j - ci * g.KH;
    const int pix = pix0 + pl;
    const uint32_t bb = udiv(pix, g.d_howo), p = pix - bb * g.Ho * g.Wo;
    const uint32_t oh = udiv(p, g.d_wo), ow = p - oh * g.Wo;
    const int ih = (int)oh * g.stride - g.pad + kh, iw0 = (int)ow * g.stride - g.pad;
    const bool hok = ih >= 0 && ih < g.H;
    const float* src = xk + bb * g.sxb + ci * g.sxc + (int64_t)ih * g.W;
    float* dst = rows + pl * RP + j * g.KW;
    for (int kw = 0; kw < g.KW; ++kw) {
      const int iw = iw0 + kw;
      dst[kw] = (hok && iw >= 0 && iw < g.W) ? src[iw] : 0.f;
    }
  }
  for (int e = threadIdx.x; e < np * (RP - R); e += THREADS) rows[(e / (RP - R)) * RP + R + e % (RP - R)] = 0.f;
  __syncthreads();
  f32x4* out = reinterpret_cast<f32x4*>(col + ((int64_t)k * N + pix0) * RP);
  const f32x4* in = reinterpret_cast<const f32x4*>(rows);
  for (int e = threadIdx.x; e < np * RP / 4; e += THREADS) out[e] = in[e];
}

// dst[k][co][RP] <- src[k][co][R] (zero pad) or the reverse (unpad) (grid: chunks x K)
__global__ __launch_bounds__(THREADS) void repad_kernel(const float* __restrict__ src, int sld, float* __restrict__ dst,
                                                        int dld, int rows, int R) {
  const int k = blockIdx.y;
  const int64_t total = (int64_t)rows * dld;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * THREADS) {
    const int row = (int)(e / dld), r = (int)(e - (int64_t)row * dld);
    dst[(int64_t)k * total + e] = r < R ? src[((int64_t)k * rows + row) * sld + r] : 0.f;
  }
}

// ---- im2col path (declared in conv_common.h) ----------------------------------
inline int padded_r(const Geom& g) { return (g.Cin * g.KH * g.KW + 3) / 4 * 4; }

bool im2col_eligible(const Geom& g) {
  const int64_t N = (int64_t)g.B * g.Ho * g.Wo;
  return padded_r(g) <= IM_MAXRP && !shape_ok(g.Cin, g.Cout) && (g.Ho * g.Wo) % 4 == 0 &&
         N * padded_r(g) * 4 < (int64_t(1) << 31) && (int64_t)g.Cout * padded_r(g) * 4 < (int64_t(1) << 31);
}

size_t im2col_workspace(const Geom& g) {
  const size_t col = align_up((size_t)g.Kc * g.B * g.Ho * g.Wo * padded_r(g) * sizeof(float), 256);
  const size_t wp = align_up((size_t)g.Kc * g.Cout * padded_r(g) * sizeof(float), 256);
  DenseFwd f; f.g = g; f.RP = padded_r(g);
  DenseWgt w; w.g = g; w.RP = padded_r(g);
  StemFwd sf; sf.g = g; sf.RP = padded_r(g);
  StemWgt sw; sw.g = g; sw.RP = padded_r(g);
  const size_t gemm = col + wp + std::max(std::max(splits_bytes(f), splits_bytes(w)), std::max(splits_bytes(sf), splits_bytes(sw)));
  return std::max(gemm, stem_eligible(g) ? stem_workspace(g) : 0);
}

static int run_im2col(const Geom& g, const float* x, float* col, hipStream_t st) {
  const int N = g.B * g.Ho * g.Wo, RP = padded_r(g);
  hipLaunchKernelGGL(im2col_kernel, dim3((unsigned)cdiv(N, IM_PB), (unsigned)g.Kc), dim3(THREADS),
                     (size_t)IM_PB * RP * sizeof(float), st, g, x, RP, col);
  return launch_status("conv im2col");
}

// FLR_STEM=col: the explicit im2col column matrix; =gather: the tiled GEMM with the
// im2col operand gathered on the fly (A/B timing); default: the direct stem
// kernels (train_stem.hip) where eligible, else the gathered GEMM.
inline bool stem_col() {
  const char* e = flr::knob("FLR_STEM");
  return e && e[0] == 'c';
}

inline bool stem_direct(const Geom& g) {
  const char* e = flr::knob("FLR_STEM");
  return !(e && (e[0] == 'c' || e[0] == 'g')) && stem_eligible(g);
}

template <class Plan>
inline void stem_divs(Plan& pl, const Geom& g) {
  pl.RR = g.Cin * g.KH * g.KW;
  pl.d_kk = conv::make_fastdiv((uint32_t)(g.KH * g.KW));
  pl.d_kw = conv::make_fastdiv((uint32_t)g.KW);
}

int fwd_im2col(const Geom& g, const float* x, const float* w, float* y, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!ws || ws_bytes < im2col_workspace(g)) return FLR_ERR_WORKSPACE;
  if (stem_direct(g)) return stem_fwd(g, x, w, y, st);
  const int RP = padded_r(g), R = g.Cin * g.KH * g.KW;
  char* base = static_cast<char*>(ws);
  float* col = reinterpret_cast<float*>(base);
  const size_t colb = align_up((size_t)g.Kc * g.B * g.Ho * g.Wo * RP * sizeof(float), 256);
  float* wp = reinterpret_cast<float*>(base + colb);
  const size_t wpb = align_up((size_t)g.Kc * g.Cout * RP * sizeof(float), 256);
  const int64_t wtot = (int64_t)g.Cout * RP;
  hipLaunchKernelGGL(repad_kernel, dim3((unsigned)std::min<int64_t>((wtot + THREADS - 1) / THREADS, 256), (unsigned)g.Kc),
                     dim3(THREADS), 0, st, w, R, wp, RP, g.Cout, R);
  int rc = launch_status("conv pad weights");
  if (rc != FLR_OK) return rc;
  if (!stem_col()) {
    StemFwd pl;
    pl.g = g; pl.RP = RP; pl.x = x; pl.wp = wp; pl.y = y;
    stem_divs(pl, g);
    return launch(pl, base + colb + wpb, ws_bytes - colb - wpb, st, "conv fwd (gathered im2col)");
  }
  if ((rc = run_im2col(g, x, col, st)) != FLR_OK) return rc;
  DenseFwd pl;
  pl.g = g; pl.RP = RP; pl.col = col; pl.wp = wp; pl.y = y;
  return launch(pl, base + colb + wpb, ws_bytes - colb - wpb, st, "conv fwd (im2col)");
}

int wgrad_im2col(const Geom& g, const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes,
                 hipStream_t st, bool have_col) {
  if (!ws || ws_bytes < im2col_workspace(g)) return FLR_ERR_WORKSPACE;
  if (stem_direct(g)) return stem_wgrad(g, x, dy, dw, ws, ws_bytes, st);
  const int RP = padded_r(g), R = g.Cin * g.KH * g.KW;
  char* base = static_cast<char*>(ws);
  float* col = reinterpret_cast<float*>(base);
  const size_t colb = align_up((size_t)g.Kc * g.B * g.Ho * g.Wo * RP * sizeof(float), 256);
  float* dwp = reinterpret_cast<float*>(base + colb);
  const size_t wpb = align_up((size_t)g.Kc * g.Cout * RP * sizeof(float), 256);
  int rc = FLR_OK;
  if (!stem_col()) {
    StemWgt pl;
    pl.g = g; pl.RP = RP; pl.x = x; pl.dy = dy; pl.dwp = dwp;
    stem_divs(pl, g);
    rc = launch(pl, base + colb + wpb, ws_bytes - colb - wpb, st, "conv bwd weight (gathered im2col)");
  } else {
    if (!have_col) rc = run_im2col(g, x, col, st);  // have_col: the forward's column matrix
    if (rc != FLR_OK) return rc;
    DenseWgt pl;
    pl.g = g; pl.RP = RP; pl.col = col; pl.dy = dy; pl.dwp = dwp;
    rc = launch(pl, base + colb + wpb, ws_bytes - colb - wpb, st, "conv bwd weight (im2col)");
  }
  if (rc != FLR_OK) return rc;
  const int64_t wtot = (int64_t)g.Cout * R;
  hipLaunchKernelGGL(repad_kernel, dim3((unsigned)std::min<int64_t>((wtot + THREADS - 1) / THREADS, 256), (unsigned)g.Kc),
                     dim3(THREADS), 0, st, dwp, RP, dw, R, g.Cout, R);
  return launch_status("conv unpad dw");
}

}  // namespace convt
}  // namespace flr

using namespace flr;

extern "C" int flr_conv2d_tap_major_ok(int64_t Cin, int64_t Cout) { return convt::shape_ok(Cin, Cout) ? 1 : 0; }

extern "C" size_t flr_conv2d_t_workspace(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                         int64_t KH, int64_t KW, int64_t stride, int64_t pad) {
  if (!convt::args_ok(K, B, Cin, H, W, Cout, KH, KW, stride, pad)) return 0;
  const conv::Geom g = conv::make_geom(K, B, Cin, H, W, Cout, KH, KW, stride, pad);
  convt::FwdT f; f.g = g;
  convt::WgtT<false> w; w.g = g;
  size_t m = std::max(convt::splits_bytes(f), convt::splits_bytes(w));
  if (stride <= 4) {
    convt::DgradT cls[convt::MAX_CLASSES];
    const int nc = convt::dgrad_classes(g, cls);
    for (int c = 0; c < nc; ++c) m = std::max(m, convt::splits_bytes(cls[c]));
  }
  return m;
}
