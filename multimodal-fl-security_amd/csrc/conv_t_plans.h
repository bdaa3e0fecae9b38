// The load plans of the tiled GEMM kernels (conv_t_kernels.h): what M, N and R
// mean for one product, how a thread loads its share of a 64 x 32 operand
// sub-tile (State / load_a / load_b: the fp32 images; State8 / load_a8 /
// load_b8: 8 consecutive k per thread, the split-at-stash images; StateT /
// load_at8 / load_bt8: the transposed images), and where an output goes.
#pragma once

#include "conv_t_prims.h"

namespace flr {
namespace convt {

struct FwdT {  // y = conv(x, W_t): M = Cout, N = B*Ho*Wo, R = ntaps*Cin
  static constexpr bool QUAD_A = false, QUAD_B = false;
  Geom g;
  const float* x;
  const float* w;
  float* y;
  int64_t wsk;  // weight floats between clients (KK*Cin*Cout; 0: every client reads one shared copy)
  static constexpr int LA = KR_VEC, LB = KR_GATHER;
  __host__ __device__ __forceinline__ int M() const { return g.Cout; }
  __host__ __device__ __forceinline__ int N() const { return g.B * g.Ho * g.Wo; }
  __host__ __device__ __forceinline__ int R() const { return g.ntaps * g.Cin; }
  // column n of the GEMM -> (image, output row, output column)
  struct Col {
    uint32_t bb, oh, ow;
  };
  __device__ __forceinline__ Col col(int n) const {
    const uint32_t bb = udiv(n, g.d_howo), p = n - bb * g.Ho * g.Wo;
    const uint32_t oh = udiv(p, g.d_wo), ow = p - oh * g.Wo;
    return Col{bb, oh, ow};
  }
  struct State {
    rsrc_t ra, rb;
    unsigned a0;            // byte offset of (k-row tid/16, m 4*(tid%16)) at tap 0, ci 0
    int ih0, iw0, xoff;     // this thread's output pixel (B operand)
    bool nok;
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    const int KK = g.KH * g.KW;
    s.ra = make_rsrc(w + (int64_t)k * wsk, (int64_t)KK * g.Cin * g.Cout);
    s.rb = make_rsrc(x + k * g.sxk, g.xext);
    s.a0 = (unsigned)(((tid / 16) * g.Cout + m0 + 4 * (tid % 16)) * 4);
    const int n = n0 + tid % 64;
    s.nok = n < N();
    const Col c = col(n);
    s.ih0 = (int)c.oh * g.stride - g.pad;
    s.iw0 = (int)c.ow * g.stride - g.pad;
    s.xoff = (int)(c.bb * g.sxb + (tid / 64) * g.sxc);
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const int slot = uni(r0 / g.Cin), ci0 = r0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    kh = uni(kh);
    kw = uni(kw);
    const int arow = ((kh * g.KW + kw) * g.Cin + ci0) * g.Cout * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 q = ld4(s.ra, s.a0, arow + i * 16 * g.Cout * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[4 * i + e] = q[e];
    }
  }
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const int slot = uni(r0 / g.Cin), ci0 = r0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    kh = uni(kh);
    kw = uni(kw);
    const int HW = (int)g.sxc;  // channel stride
    const int ih = s.ih0 + kh, iw = s.iw0 + kw;
    // bitwise & (no short-circuit): the gather stays branch-free, one basic block with the MFMAs
    const bool ok = s.nok & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
    const unsigned addr = (unsigned)((s.xoff + ih * g.W + iw) * 4);
    const unsigned vb = ok ? addr : SENT;
    const int cb = ci0 * HW * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = ld1(s.rb, vb, cb + i * 4 * HW * 4);
  }
  // y[k][m][n]: n = b*Ho*Wo + p is linear in the [K][C][B][Ho][Wo] layout
  __device__ __forceinline__ void store(int k, int m, int n, float v) const { y[k * g.syk + m * g.syc + n] = v; }
  __device__ __forceinline__ bool linear() const { return true; }
  __device__ __forceinline__ float* out() const { return y; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return k * g.syk + m0 * g.syc + n0; }
  __device__ __forceinline__ int64_t ldm() const { return g.syc; }
  // ---- k-contiguous loads for the split-at-stash kernel: thread (row = tid & 63,
  // k = 8 (tid >> 6) .. +7) of a 64 x 32 sub-tile
  using State8 = State;  // the same fields, filled for the k-contiguous mapping
  __device__ __forceinline__ State8 init8(int k, int m0, int n0, int tid) const {
    State8 s;
    const int KK = g.KH * g.KW;
    const int row = tid & 63, k0 = 8 * (tid >> 6);
    s.ra = make_rsrc(w + (int64_t)k * wsk, (int64_t)KK * g.Cin * g.Cout);
    s.rb = make_rsrc(x + k * g.sxk, g.xext);
    s.a0 = (unsigned)((k0 * g.Cout + m0 + row) * 4);
    const int n = n0 + row;
    s.nok = n < N();
    const Col c = col(n);
    s.ih0 = (int)c.oh * g.stride - g.pad;
    s.iw0 = (int)c.ow * g.stride - g.pad;
    s.xoff = (int)(c.bb * g.sxb + k0 * g.sxc);
    return s;
  }
  __device__ __forceinline__ void load_a8(const State8& s, int r0, float (&a)[8]) const {  // A(co, ci): lanes along co
    const int slot = uni((int)udiv((uint32_t)r0, g.d_cin)), ci0 = r0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    const int arow = uni(((kh * g.KW + kw) * g.Cin + ci0) * g.Cout * 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = ld1(s.ra, s.a0, arow + e * g.Cout * 4);
  }
  __device__ __forceinline__ void load_b8(const State8& s, int r0, float (&b)[8]) const {  // B(pixel, ci): 8 channels
    const int slot = uni((int)udiv((uint32_t)r0, g.d_cin)), ci0 = r0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    kh = uni(kh);
    kw = uni(kw);
    const int HW = (int)g.sxc;
    const int ih = s.ih0 + kh, iw = s.iw0 + kw;
    const bool ok = s.nok & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
    const unsigned addr = (unsigned)((s.xoff + ih * g.W + iw) * 4);
    const unsigned vb = ok ? addr : SENT;
    const int cb = ci0 * HW * 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = ld1(s.rb, vb, cb + e * HW * 4);
  }
  // ---- the resident-B form (rgemm_kernel: stride 1, Ho == H, Wo == W): the B operand
  // of a column at no tap shift (load_b8's address at the centre tap, channel 0: float
  // offset in the client's x; (oh, ow) its pixel), the channel stride, and a reduction
  // slot's shift of that pixel
  __host__ __device__ __forceinline__ int Cr() const { return g.Cin; }  // reduction channels per tap
  __device__ __forceinline__ rsrc_t res_rsrc(int k) const { return make_rsrc(x + k * g.sxk, g.xext); }
  __device__ __forceinline__ int res_cs() const { return (int)g.sxc; }
  __device__ __forceinline__ int res_col(int n, int& oh, int& ow) const {
    const Col c = col(n);
    oh = (int)c.oh;
    ow = (int)c.ow;
    return (int)(c.bb * g.sxb) + oh * g.W + ow;
  }
  __device__ __forceinline__ void res_shift(int slot, int& dh, int& dw) const {
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    dh = kh - g.pad;
    dw = kw - g.pad;
  }
};

// dx = conv^T(dy, W_t) over ONE stride-parity class of input pixels:
// ih = ca + stride*ihc, iw = cb + stride*iwc.  Only the taps kh = (ih + pad)
// mod stride (same for kw) reach such a pixel, so a class is a dense GEMM
// M = Cin, N = B*Hc*Wc, R = ntc*Cout with no zero-padded taps — a stride-2
// dgrad runs the four classes and does the fwd's MFMA work, not four times
// it.  Stride 1 is the single class (0, 0) with every live tap.
struct DgradT {
  static constexpr bool QUAD_A = true, QUAD_B = false;
  Geom g;
  const float* dy;
  const float* w;
  float* dx;
  const float* add;  // optional addend in dx's layout: dx = dgrad + add (one rounding)
  int64_t wsk;       // weight floats between clients (KK*Cin*Cout; 0: one shared copy)
  int ca, cb, Hc, Wc, ntc;
  conv::FastDiv d_hcwc, d_wc;
  int8_t ckh[conv::MAXTAPS], ckw[conv::MAXTAPS];
  conv::TapRect crect;  // the class taps: a rectangle of step = stride
  static constexpr int LA = RK_VEC, LB = KR_GATHER;
  __host__ __device__ __forceinline__ int M() const { return g.Cin; }
  __host__ __device__ __forceinline__ int N() const { return g.B * Hc * Wc; }
  __host__ __device__ __forceinline__ int R() const { return ntc * g.Cout; }
  // column n of the class's GEMM -> (image, row, column) in the class's Hc x Wc grid
  struct Col {
    uint32_t bb, ihc, iwc;
  };
  __device__ __forceinline__ Col col(int n) const {
    const uint32_t bb = udiv(n, d_hcwc), p = n - bb * Hc * Wc;
    const uint32_t ihc = udiv(p, d_wc), iwc = p - ihc * Wc;
    return Col{bb, ihc, iwc};
  }
  struct State {
    rsrc_t ra, rb;
    unsigned a0;
    int ih, iw, yoff;  // ih, iw: this lane's input pixel + pad
    bool nok;
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    const int KK = g.KH * g.KW;
    s.ra = make_rsrc(w + (int64_t)k * wsk, (int64_t)KK * g.Cin * g.Cout);
    s.rb = make_rsrc(dy + k * g.syk, g.yext);
    s.a0 = (unsigned)(((m0 + tid / 8) * g.Cout + 4 * (tid % 8)) * 4);
    const int n = n0 + tid % 64;
    s.nok = n < N();
    const Col c = col(n);
    s.ih = ca + (int)c.ihc * g.stride + g.pad;
    s.iw = cb + (int)c.iwc * g.stride + g.pad;
    s.yoff = (int)(c.bb * g.syb + (tid / 64) * g.syc);
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const int slot = uni(r0 / g.Cout), co0 = r0 - slot * g.Cout;
    int kh, kw;
    conv::rect_tap(crect, slot, kh, kw);
    kh = uni(kh);
    kw = uni(kw);
    const int abase = ((kh * g.KW + kw) * g.Cin * g.Cout + co0) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 q = ld4(s.ra, s.a0, abase + i * 32 * g.Cout * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[4 * i + e] = q[e];
    }
  }
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const int slot = uni(r0 / g.Cout), co0 = r0 - slot * g.Cout;
    int kh, kw;
    conv::rect_tap(crect, slot, kh, kw);
    kh = uni(kh);
    kw = uni(kw);
    // the class guarantees (ih + pad - kh) % stride == 0
    const int nh = s.ih - kh, nw = s.iw - kw;
    const int oh = g.stride == 1 ? nh : nh / g.stride, ow = g.stride == 1 ? nw : nw / g.stride;
    const bool ok = s.nok & (nh >= 0) & (nw >= 0) & (oh < g.Ho) & (ow < g.Wo);
    const unsigned addr = (unsigned)((s.yoff + oh * g.Wo + ow) * 4);
    const unsigned vb = ok ? addr : SENT;
    const int cs = (int)g.syc;  // channel stride
    const int cb0 = co0 * cs * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = ld1(s.rb, vb, cb0 + i * 4 * cs * 4);
  }
  __device__ __forceinline__ int64_t index(int k, int m, int n) const {  // dx offset of output (m, n) of client k
    const Col c = col(n);
    const int ih = ca + (int)c.ihc * g.stride, iw = cb + (int)c.iwc * g.stride;
    return k * g.sxk + m * g.sxc + c.bb * g.sxb + ih * g.W + iw;
  }
  __device__ __forceinline__ void store(int k, int m, int n, float v) const {
    const int64_t i = index(k, m, n);
    dx[i] = add ? __fadd_rn(v, add[i]) : v;
  }
  // stride 1 (the one class is every pixel): dx[k][m][n] is linear in n
  __device__ __forceinline__ bool linear() const { return g.stride == 1; }
  __device__ __forceinline__ float* out() const { return dx; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return k * g.sxk + m0 * g.sxc + n0; }
  __device__ __forceinline__ int64_t ldm() const { return g.sxc; }
  using State8 = State;  // the same fields, filled for the k-contiguous mapping
  __device__ __forceinline__ State8 init8(int k, int m0, int n0, int tid) const {
    State8 s;
    const int KK = g.KH * g.KW;
    const int row = tid & 63, k0 = 8 * (tid >> 6);
    s.ra = make_rsrc(w + (int64_t)k * wsk, (int64_t)KK * g.Cin * g.Cout);
    s.rb = make_rsrc(dy + k * g.syk, g.yext);
    // A = W(ci, co) is k-contiguous: quad lanes (stash_row / stash_k, QUAD_A)
    s.a0 = (unsigned)(((m0 + stash_row<QUAD_A>(tid)) * g.Cout + stash_k<QUAD_A>(tid)) * 4);
    const int n = n0 + row;
    s.nok = n < N();
    const Col c = col(n);
    s.ih = ca + (int)c.ihc * g.stride + g.pad;
    s.iw = cb + (int)c.iwc * g.stride + g.pad;
    s.yoff = (int)(c.bb * g.syb + k0 * g.syc);
    return s;
  }
  __device__ __forceinline__ void load_a8(const State8& s, int r0, float (&a)[8]) const {  // A(ci, co): 8 consecutive co
    const int slot = uni((int)udiv((uint32_t)r0, g.d_cout)), co0 = r0 - slot * g.Cout;
    int kh, kw;
    conv::rect_tap(crect, slot, kh, kw);
    const int abase = uni(((kh * g.KW + kw) * g.Cin * g.Cout + co0) * 4);
    const f32x4 q0 = ld4(s.ra, s.a0, abase), q1 = ld4(s.ra, s.a0, abase + 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = q0[e];
      a[4 + e] = q1[e];
    }
  }
  __device__ __forceinline__ void load_b8(const State8& s, int r0, float (&b)[8]) const {  // B(input pixel, co): 8 channels
    const int slot = uni((int)udiv((uint32_t)r0, g.d_cout)), co0 = r0 - slot * g.Cout;
    int kh, kw;
    conv::rect_tap(crect, slot, kh, kw);
    kh = uni(kh);
    kw = uni(kw);
    const int nh = s.ih - kh, nw = s.iw - kw;
    const int oh = g.stride == 1 ? nh : nh / g.stride, ow = g.stride == 1 ? nw : nw / g.stride;
    const bool ok = s.nok & (nh >= 0) & (nw >= 0) & (oh < g.Ho) & (ow < g.Wo);
    const unsigned addr = (unsigned)((s.yoff + oh * g.Wo + ow) * 4);
    const unsigned vb = ok ? addr : SENT;
    const int cs = (int)g.syc;
    const int cb0 = co0 * cs * 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = ld1(s.rb, vb, cb0 + e * cs * 4);
  }
  // ---- the resident-B form (rgemm_kernel; stride 1, the one class, Ho == H, Wo == W):
  // as FwdT's hooks, on dy — a slot reads output pixel (ih + pad - kh, iw + pad - kw)
  __host__ __device__ __forceinline__ int Cr() const { return g.Cout; }
  __device__ __forceinline__ rsrc_t res_rsrc(int k) const { return make_rsrc(dy + k * g.syk, g.yext); }
  __device__ __forceinline__ int res_cs() const { return (int)g.syc; }
  __device__ __forceinline__ int res_col(int n, int& oh, int& ow) const {
    const Col c = col(n);
    oh = (int)c.ihc;
    ow = (int)c.iwc;
    return (int)(c.bb * g.syb) + oh * g.Wo + ow;
  }
  __device__ __forceinline__ void res_shift(int slot, int& dh, int& dw) const {
    int kh, kw;
    conv::rect_tap(crect, slot, kh, kw);
    dh = g.pad - kh;
    dw = g.pad - kw;
  }
};

// The parity classes of a dgrad (stride^2 of them, fewer when H or W < stride).
inline int dgrad_classes(const Geom& g, DgradT* out) {
  int n = 0;
  for (int ca = 0; ca < std::min(g.stride, g.H); ++ca)
    for (int cb = 0; cb < std::min(g.stride, g.W); ++cb) {
      DgradT& c = out[n++];
      c.g = g;
      c.ca = ca;
      c.cb = cb;
      c.Hc = (g.H - ca + g.stride - 1) / g.stride;
      c.Wc = (g.W - cb + g.stride - 1) / g.stride;
      c.d_hcwc = conv::make_fastdiv((uint32_t)(c.Hc * c.Wc));
      c.d_wc = conv::make_fastdiv((uint32_t)c.Wc);
      c.ntc = 0;
      for (int t = 0; t < g.ntaps; ++t) {
        const int kh = g.tap_kh[t], kw = g.tap_kw[t];
        if (((ca + g.pad - kh) % g.stride + g.stride) % g.stride != 0) continue;
        if (((cb + g.pad - kw) % g.stride + g.stride) % g.stride != 0) continue;
        c.ckh[c.ntc] = (int8_t)kh;
        c.ckw[c.ntc] = (int8_t)kw;
        ++c.ntc;
      }
      c.crect = conv::make_rect(c.ckh, c.ckw, c.ntc, g.stride);
    }
  return n;
}
constexpr int MAX_CLASSES = 16;

// dW_t[tap][ci][co] = sum_q x(q; tap, ci) dy(q; co): M = ntaps*Cin (slot, ci),
// N = Cout, R = B*Ho*Wo.  A 64-row m-tile lies inside one tap (Cin % 64 == 0).
template <bool BVEC>
struct WgtT {
  static constexpr bool QUAD_A = false, QUAD_B = false;
  Geom g;
  const float* x;
  const float* dy;
  float* dw;
  // optional clip-norm partials (flr_conv2d_bwd_weight_t_sq): one fp64 sum of
  // squares per output tile (split-K 1) or per 256-value treduce block, at
  // sq[k * sq_ld + slot] — the optimizer's clip norm then never re-reads dw
  double* sq = nullptr;
  int sq_ld = 0;
  static constexpr int LA = RK_GATHER, LB = BVEC ? RK_VEC : RK_GATHER;
  __host__ __device__ __forceinline__ int M() const { return g.ntaps * g.Cin; }
  __host__ __device__ __forceinline__ int N() const { return g.Cout; }
  __host__ __device__ __forceinline__ int R() const { return g.B * g.Ho * g.Wo; }
  struct State {
    rsrc_t ra, rb;
    int kh, kw, aoff, boff;
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    s.ra = make_rsrc(x + k * g.sxk, g.xext);
    s.rb = make_rsrc(dy + k * g.syk, g.yext);
    const int slot = uni(m0 / g.Cin), ci0 = m0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    s.kh = uni(kh);
    s.kw = uni(kw);
    s.aoff = (int)((ci0 + tid / 32) * g.sxc);
    s.boff = (int)((BVEC ? (n0 + tid / 8) : (n0 + tid / 32)) * g.syc);
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const int tid = threadIdx.x;
    const int HoWo = g.Ho * g.Wo, R = this->R();
    {  // A: x gathered at q = r0 + tid % 32
      const int q = r0 + tid % 32;
      const uint32_t bb = udiv(q, g.d_howo), p = q - bb * HoWo;
      const uint32_t oh = udiv(p, g.d_wo), ow = p - oh * g.Wo;
      const int ih = (int)oh * g.stride - g.pad + s.kh, iw = (int)ow * g.stride - g.pad + s.kw;
      const bool ok = (q < R) & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
      const unsigned addr = (unsigned)(((int)(bb * g.sxb) + s.aoff + ih * g.W + iw) * 4);
      const unsigned va = ok ? addr : SENT;
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = ld1(s.ra, va, i * 8 * (int)g.sxc * 4);
    }
  }
  // B: dy[co][q] with q = b*Ho*Wo + p contiguous per channel ([K][C][B][Ho][Wo])
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const int tid = threadIdx.x, R = this->R();
    if constexpr (BVEC) {  // q = r0 + 4 (tid % 8) .. +3
      const int q = r0 + 4 * (tid % 8);
      const unsigned vb = q < R ? (unsigned)((s.boff + q) * 4) : SENT;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 v = ld4(s.rb, vb, i * 32 * (int)g.syc * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) b[4 * i + e] = v[e];
      }
    } else {  // q = r0 + tid % 32
      const int q = r0 + tid % 32;
      const unsigned vb = q < R ? (unsigned)((s.boff + q) * 4) : SENT;
#pragma unroll
      for (int i = 0; i < 8; ++i) b[i] = ld1(s.rb, vb, i * 8 * (int)g.syc * 4);
    }
  }
  __device__ __forceinline__ void store(int k, int m, int n, float v) const {
    const int slot = (int)udiv(m, g.d_cin), ci = m - slot * g.Cin;
    dw[(((int64_t)k * g.KH * g.KW + tap_index(g, slot)) * g.Cin + ci) * g.Cout + n] = v;
  }
  __device__ __forceinline__ bool linear() const { return true; }
  __device__ __forceinline__ float* out() const { return dw; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const {
    const int slot = m0 / g.Cin, ci0 = m0 - slot * g.Cin;
    return (((int64_t)k * g.KH * g.KW + tap_index(g, slot)) * g.Cin + ci0) * g.Cout + n0;
  }
  __device__ __forceinline__ int64_t ldm() const { return g.Cout; }
  struct State8 {
    rsrc_t ra, rb;
    int kh, kw, k0;
    unsigned aoff, boff;
  };
  __device__ __forceinline__ State8 init8(int k, int m0, int n0, int tid) const {
    State8 s;
    s.ra = make_rsrc(x + k * g.sxk, g.xext);
    s.rb = make_rsrc(dy + k * g.syk, g.yext);
    const int slot = uni(m0 / g.Cin), ci0 = m0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    s.kh = uni(kh);
    s.kw = uni(kw);
    const int row = tid & 63;
    s.k0 = uni(8 * (tid >> 6));  // the wave's k-group: its 8 pixels are wave-uniform
    s.aoff = (unsigned)((ci0 + row) * g.sxc * 4);
    s.boff = (unsigned)((n0 + row) * g.syc * 4);
    return s;
  }
  // A(ci, pixel q): the 8 pixels of the wave's k-group are wave-uniform, so their
  // decomposition and padding test run on the scalar unit (soffset per pixel)
  __device__ __forceinline__ void load_a8(const State8& s, int r0, float (&a)[8]) const {
    const int R = this->R(), HoWo = g.Ho * g.Wo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int q = uni(r0 + s.k0 + e);
      const int bb = uni((int)udiv((uint32_t)q, g.d_howo)), p = q - bb * HoWo;
      const int oh = uni((int)udiv((uint32_t)p, g.d_wo)), ow = p - oh * g.Wo;
      const int ih = oh * g.stride - g.pad + s.kh, iw = ow * g.stride - g.pad + s.kw;
      const bool ok = (q < R) & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
      const int soff = uni(ok ? (bb * (int)g.sxb + ih * g.W + iw) * 4 : 0);
      a[e] = ld1(s.ra, ok ? s.aoff : SENT, soff);
    }
  }
  // B(co, q): dy[co][q], q contiguous per channel
  __device__ __forceinline__ void load_b8(const State8& s, int r0, float (&b)[8]) const {
    const int R = this->R();
    const int q0 = r0 + s.k0;
    if constexpr (BVEC) {  // syc % 4 == 0, R % 4 == 0
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = q0 + 4 * i < R;
        const f32x4 v = ld4(s.rb, ok ? s.boff + (unsigned)((q0 + 4 * i) * 4) : SENT, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) b[4 * i + e] = v[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = ld1(s.rb, (q0 + e < R) ? s.boff + (unsigned)((q0 + e) * 4) : SENT, 0);
    }
  }
  // ---- transposed-image loads (wsgemm_kernel): thread t holds rows 8 (t >> 5) .. +7 of
  // the 64-row sub-tile at reduction index k = t & 31 — the 32 lanes of a half-wave
  // read 32 consecutive pixels of one row (128 B), and the thread's 8 values are
  // the 8 consecutive rows of one k, one 16-B chunk of a [k][row] LDS image
  struct StateT {
    rsrc_t ra, rb;
    int kh, kw;
    unsigned arow, brow;
  };
  __device__ __forceinline__ StateT initT(int k, int m0, int n0, int tid) const {
    StateT s;
    s.ra = make_rsrc(x + k * g.sxk, g.xext);
    s.rb = make_rsrc(dy + k * g.syk, g.yext);
    const int slot = uni(m0 / g.Cin), ci0 = m0 - slot * g.Cin;
    int kh, kw;
    slot_tap(g, slot, kh, kw);
    s.kh = uni(kh);
    s.kw = uni(kw);
    const int rg = tid >> 5;
    s.arow = (unsigned)((ci0 + 8 * rg) * g.sxc * 4);
    s.brow = (unsigned)((n0 + 8 * rg) * g.syc * 4);
    return s;
  }
  __device__ __forceinline__ void load_at8(const StateT& s, int r0, float (&a)[8]) const {  // x(ci, pixel q of tap (kh, kw))
    const int q = r0 + (int)(threadIdx.x & 31), HoWo = g.Ho * g.Wo;
    const uint32_t bb = udiv(q, g.d_howo), p = q - bb * HoWo;
    const uint32_t oh = udiv(p, g.d_wo), ow = p - oh * g.Wo;
    const int ih = (int)oh * g.stride - g.pad + s.kh, iw = (int)ow * g.stride - g.pad + s.kw;
    const bool ok = (q < R()) & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
    const unsigned va = ok ? s.arow + (unsigned)(((int)(bb * g.sxb) + ih * g.W + iw) * 4) : SENT;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = ld1(s.ra, va, i * (int)g.sxc * 4);
  }
  __device__ __forceinline__ void load_bt8(const StateT& s, int r0, float (&b)[8]) const {  // dy(co, q), q contiguous
    const int q = r0 + (int)(threadIdx.x & 31);
    const unsigned vb = q < R() ? s.brow + (unsigned)(q * 4) : SENT;
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = ld1(s.rb, vb, i * (int)g.syc * 4);
  }
};

// ---- explicit im2col (short reductions: the stem) -----------------------------
// col[k][pix][RP], pix = b*Ho*Wo + oh*Wo + ow, r = (ci*KH + kh)*KW + kw (torch
// weight order), zero for padding taps and for r >= R (RP = R rounded up to 4).
// The weights are used as wp[k][co][RP] (a zero-padded copy), so both GEMM
// operands are k-contiguous rows and load as 16-B vectors.
struct DenseFwd {  // y[co][pix] = sum_r wp[co][r] col[pix][r]: M = Cout, N = B*Ho*Wo, R = RP
  Geom g;
  int RP;
  const float* col;
  const float* wp;
  float* y;
  static constexpr int LA = RK_VEC, LB = RK_VEC;
  __host__ __device__ __forceinline__ int M() const { return g.Cout; }
  __host__ __device__ __forceinline__ int N() const { return g.B * g.Ho * g.Wo; }
  __host__ __device__ __forceinline__ int R() const { return RP; }
  struct State {
    rsrc_t ra, rb;
    unsigned a0, b0;
    bool aok[2], bok[2];
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    s.ra = make_rsrc(wp + (int64_t)k * g.Cout * RP, (int64_t)g.Cout * RP);
    s.rb = make_rsrc(col + (int64_t)k * N() * RP, (int64_t)N() * RP);
    s.a0 = (unsigned)(((m0 + tid / 8) * RP + 4 * (tid % 8)) * 4);
    s.b0 = (unsigned)(((n0 + tid / 8) * RP + 4 * (tid % 8)) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      s.aok[i] = m0 + tid / 8 + 32 * i < M();
      s.bok[i] = n0 + tid / 8 + 32 * i < N();
    }
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const bool kok = r0 + 4 * (int)(threadIdx.x % 8) < RP;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 qa = ld4(s.ra, (kok && s.aok[i]) ? s.a0 + (unsigned)((r0 + 32 * i * RP) * 4) : SENT, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[4 * i + e] = qa[e];
    }
  }
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const bool kok = r0 + 4 * (int)(threadIdx.x % 8) < RP;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 qb = ld4(s.rb, (kok && s.bok[i]) ? s.b0 + (unsigned)((r0 + 32 * i * RP) * 4) : SENT, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) b[4 * i + e] = qb[e];
    }
  }
  // y[k][m][n]: n = b*Ho*Wo + p is linear in the [K][C][B][Ho][Wo] layout
  __device__ __forceinline__ void store(int k, int m, int n, float v) const { y[k * g.syk + m * g.syc + n] = v; }
  __device__ __forceinline__ bool linear() const { return true; }
  __device__ __forceinline__ float* out() const { return y; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return k * g.syk + m0 * g.syc + n0; }
  __device__ __forceinline__ int64_t ldm() const { return g.syc; }
};

struct DenseWgt {  // dwp[co][r] = sum_pix dy[co][pix] col[pix][r]: M = Cout, N = RP, R = B*Ho*Wo (HoWo % 4 == 0)
  Geom g;
  int RP;
  const float* col;
  const float* dy;
  float* dwp;
  static constexpr int LA = RK_VEC, LB = KR_VEC;
  __host__ __device__ __forceinline__ int M() const { return g.Cout; }
  __host__ __device__ __forceinline__ int N() const { return RP; }
  __host__ __device__ __forceinline__ int R() const { return g.B * g.Ho * g.Wo; }
  struct State {
    rsrc_t ra, rb;
    int arow;
    bool aok[2], nok;
    unsigned b0;
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    s.ra = make_rsrc(dy + k * g.syk, g.yext);
    s.rb = make_rsrc(col + (int64_t)k * R() * RP, (int64_t)R() * RP);
    s.arow = (int)((m0 + tid / 8) * g.syc);
#pragma unroll
    for (int i = 0; i < 2; ++i) s.aok[i] = m0 + tid / 8 + 32 * i < M();
    const int n = n0 + 4 * (tid % 16);
    s.nok = n < RP;
    s.b0 = (unsigned)(((tid / 16) * RP + n) * 4);
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const int tid = threadIdx.x, R = this->R();
    const int q = r0 + 4 * (tid % 8);  // dy[co][q]: q = b*Ho*Wo + p contiguous per channel
    const unsigned va = (unsigned)((s.arow + q) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 qa = ld4(s.ra, (q < R && s.aok[i]) ? va + (unsigned)(i * 32 * (int)g.syc * 4) : SENT, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[4 * i + e] = qa[e];
    }
  }
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const int tid = threadIdx.x, R = this->R();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pix = r0 + tid / 16 + 16 * i;
      const f32x4 qb = ld4(s.rb, (pix < R && s.nok) ? s.b0 + (unsigned)((r0 + 16 * i) * RP * 4) : SENT, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) b[4 * i + e] = qb[e];
    }
  }
  __device__ __forceinline__ void store(int k, int m, int n, float v) const { dwp[((int64_t)k * g.Cout + m) * RP + n] = v; }
  __device__ __forceinline__ bool linear() const { return true; }
  __device__ __forceinline__ float* out() const { return dwp; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return ((int64_t)k * g.Cout + m0) * RP + n0; }
  __device__ __forceinline__ int64_t ldm() const { return RP; }
};

// The same two GEMMs with the im2col operand gathered on the fly from x
// ([K][C][B][H][W]; one client's image batch, 393 KB at the C3 stem, stays in
// L2 across its 49 taps): no column matrix is written or read.  Reduction
// index r = (ci*KH + kh)*KW + kw (torch weight order), zero past R = Cin*KH*KW.
struct StemFwd {  // y[co][pix] = sum_r wp[co][r] x(pix; r): M = Cout, N = B*Ho*Wo, R = RP
  Geom g;
  int RP, RR;  // RR = Cin*KH*KW
  conv::FastDiv d_kk, d_kw;
  const float* x;
  const float* wp;
  float* y;
  static constexpr int LA = RK_VEC, LB = KR_GATHER;
  __host__ __device__ __forceinline__ int M() const { return g.Cout; }
  __host__ __device__ __forceinline__ int N() const { return g.B * g.Ho * g.Wo; }
  __host__ __device__ __forceinline__ int R() const { return RP; }
  struct State {
    rsrc_t ra, rb;
    unsigned a0;
    bool aok[2], nok;
    int ih0, iw0, xoff;
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    s.ra = make_rsrc(wp + (int64_t)k * g.Cout * RP, (int64_t)g.Cout * RP);
    s.a0 = (unsigned)(((m0 + tid / 8) * RP + 4 * (tid % 8)) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) s.aok[i] = m0 + tid / 8 + 32 * i < M();
    s.rb = make_rsrc(x + k * g.sxk, g.xext);
    const int n = n0 + tid % 64;
    s.nok = n < N();
    const uint32_t bb = udiv(n, g.d_howo), p = n - bb * g.Ho * g.Wo;
    const uint32_t oh = udiv(p, g.d_wo), ow = p - oh * g.Wo;
    s.ih0 = (int)oh * g.stride - g.pad;
    s.iw0 = (int)ow * g.stride - g.pad;
    s.xoff = (int)(bb * g.sxb);
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const bool kok = r0 + 4 * (int)(threadIdx.x % 8) < RP;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 qa = ld4(s.ra, (kok && s.aok[i]) ? s.a0 + (unsigned)((r0 + 32 * i * RP) * 4) : SENT, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[4 * i + e] = qa[e];
    }
  }
  // k-row tid/64 + 4i is the wave's: (ci, kh, kw) are wave-uniform (SGPRs)
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const int KK = g.KH * g.KW;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = uni(r0 + (int)(threadIdx.x / 64) + 4 * i);
      const int ci = uni((int)udiv((uint32_t)r, d_kk)), rem = r - ci * KK;
      const int kh = uni((int)udiv((uint32_t)rem, d_kw)), kw = rem - kh * g.KW;
      const int ih = s.ih0 + kh, iw = s.iw0 + kw;
      const bool ok = s.nok & (r < RR) & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
      const unsigned addr = (unsigned)((s.xoff + ih * g.W + iw) * 4);
      const unsigned vb = ok ? addr : SENT;
      b[i] = ld1(s.rb, vb, uni(ci * (int)g.sxc * 4));
    }
  }
  __device__ __forceinline__ void store(int k, int m, int n, float v) const { y[k * g.syk + m * g.syc + n] = v; }
  __device__ __forceinline__ bool linear() const { return true; }
  __device__ __forceinline__ float* out() const { return y; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return k * g.syk + m0 * g.syc + n0; }
  __device__ __forceinline__ int64_t ldm() const { return g.syc; }
};

struct StemWgt {  // dwp[co][r] = sum_pix dy[co][pix] x(pix; r): M = Cout, N = RP, R = B*Ho*Wo (HoWo % 4 == 0)
  Geom g;
  int RP, RR;
  conv::FastDiv d_kk, d_kw;
  const float* x;
  const float* dy;
  float* dwp;
  static constexpr int LA = RK_VEC, LB = KR_VEC;
  __host__ __device__ __forceinline__ int M() const { return g.Cout; }
  __host__ __device__ __forceinline__ int N() const { return RP; }
  __host__ __device__ __forceinline__ int R() const { return g.B * g.Ho * g.Wo; }
  struct State {
    rsrc_t ra, rb;
    int arow;
    bool aok[2];
    int roff[4];          // this thread's 4 reduction columns r: ci*sxc + kh*W + kw
    int8_t kh[4], kw[4];  // (kh = -128: r past R)
  };
  __device__ __forceinline__ State init(int k, int m0, int n0, int tid) const {
    State s;
    s.ra = make_rsrc(dy + k * g.syk, g.yext);
    s.arow = (int)((m0 + tid / 8) * g.syc);
#pragma unroll
    for (int i = 0; i < 2; ++i) s.aok[i] = m0 + tid / 8 + 32 * i < M();
    s.rb = make_rsrc(x + k * g.sxk, g.xext);
    const int KK = g.KH * g.KW;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = n0 + 4 * (tid % 16) + e;
      const int ci = (int)udiv((uint32_t)r, d_kk), rem = r - ci * KK;
      const int kh = (int)udiv((uint32_t)rem, d_kw), kw = rem - kh * g.KW;
      const bool ok = r < RR;
      s.kh[e] = ok ? (int8_t)kh : (int8_t)-128;
      s.kw[e] = (int8_t)kw;
      s.roff[e] = ok ? ci * (int)g.sxc + kh * g.W + kw : 0;
    }
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&a)[8]) const {
    const int tid = threadIdx.x, R = this->R();
    const int q = r0 + 4 * (tid % 8);  // dy[co][q]: q = b*Ho*Wo + p contiguous per channel
    const unsigned va = (unsigned)((s.arow + q) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f32x4 qa = ld4(s.ra, (q < R && s.aok[i]) ? va + (unsigned)(i * 32 * (int)g.syc * 4) : SENT, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[4 * i + e] = qa[e];
    }
  }
  // KR_VEC image: pixel k-rows tid/16 + 16i, columns r = n0 + 4 (tid % 16) + e
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&b)[8]) const {
    const int tid = threadIdx.x, R = this->R(), HoWo = g.Ho * g.Wo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = r0 + tid / 16 + 16 * i;
      const uint32_t bb = udiv((uint32_t)q, g.d_howo), p = (uint32_t)q - bb * HoWo;
      const uint32_t oh = udiv(p, g.d_wo), ow = p - oh * g.Wo;
      const int ih0 = (int)oh * g.stride - g.pad, iw0 = (int)ow * g.stride - g.pad;
      const int base = (int)(bb * g.sxb) + ih0 * g.W + iw0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ih = ih0 + s.kh[e], iw = iw0 + s.kw[e];
        const bool ok = (q < R) & (s.kh[e] >= 0) & (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W);
        const unsigned addr = (unsigned)((base + s.roff[e]) * 4);
        b[4 * i + e] = ld1(s.rb, ok ? addr : SENT, 0);
      }
    }
  }
  __device__ __forceinline__ void store(int k, int m, int n, float v) const { dwp[((int64_t)k * g.Cout + m) * RP + n] = v; }
  __device__ __forceinline__ bool linear() const { return true; }
  __device__ __forceinline__ float* out() const { return dwp; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return ((int64_t)k * g.Cout + m0) * RP + n0; }
  __device__ __forceinline__ int64_t ldm() const { return RP; }
};

// ---- batched dense GEMM (the text branch and the late-fusion MLP) -------------
// C_k[m][n] = (bias_k[n] | add_k[m][n]) + sum_r A_k(m, r) B_k(n, r) for every
// client k, with arbitrary strides: A(m, r) at a + k a_k + m a_m + r a_r, etc.
// Operand modes: RK (r contiguous: 16-B loads along r), KR (m / n contiguous:
// 16-B loads along the row index), G (anything else: scalar gathers).  Same
// tiled exact-fp32 MFMA kernel and split-K rule as the convolutions, so a
// client's result never depends on how many clients share the launch.
struct BatchDim {
  int Kc;
};
enum BMode { BM_RK = 0, BM_KR = 1, BM_G = 2 };

struct BGemmArgs {
  BatchDim g;
  int m, n, r;
  const float* a;
  int64_t a_k, a_m, a_r, a_ext;
  const float* b;
  int64_t b_k, b_n, b_r, b_ext;
  float* c;
  int64_t c_k, c_m, c_n;
  const float* bias;  // bias[k * bias_k + n]
  int64_t bias_k;
  const float* add;   // add[k*c_k + m*c_m + n*c_n] (may alias c)
  // epilogue (flr_bgemm_ex): pre <- v; v <- act(v [, aux]); v <- v * mul
  int act;            // FLR_ACT_*
  const float* mul;   // indexed like c (may be NULL)
  const float* aux;   // indexed like c: the saved activation input/output of the D* modes
  float* pre;         // indexed like c: the pre-activation value (may be NULL)
};

// exact-erf GELU as torch's CPU kernel: x * 0.5 * (1 + erf(x * M_SQRT1_2))
__device__ __forceinline__ float gelu_erf(float x) {
  return __fmul_rn(__fmul_rn(x, 0.5f), __fadd_rn(1.f, erff(__fmul_rn(x, 0.70710678118654752440f))));
}
// d/dx GELU: 0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi)
__device__ __forceinline__ float gelu_erf_grad(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
  const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;
  return cdf + x * pdf;
}

// the activation given the aux value (the D* modes' saved input / output)
__device__ __forceinline__ float apply_act_v(int act, float v, float ax) {
  switch (act) {
    case FLR_ACT_RELU: return v > 0.f ? v : 0.f;
    case FLR_ACT_GELU: return gelu_erf(v);
    case FLR_ACT_TANH: return tanhf(v);
    case FLR_ACT_DRELU: return ax > 0.f ? v : 0.f;
    case FLR_ACT_DGELU: return v * gelu_erf_grad(ax);
    case FLR_ACT_DTANH: return v * (1.f - ax * ax);
    default: return v;
  }
}

__device__ __forceinline__ float apply_act(int act, float v, const float* aux, int64_t i) {
  switch (act) {
    case FLR_ACT_RELU: return v > 0.f ? v : 0.f;
    case FLR_ACT_GELU: return gelu_erf(v);
    case FLR_ACT_TANH: return tanhf(v);
    case FLR_ACT_DRELU: return aux[i] > 0.f ? v : 0.f;
    case FLR_ACT_DGELU: return v * gelu_erf_grad(aux[i]);
    case FLR_ACT_DTANH: { const float y = aux[i]; return v * (1.f - y * y); }
    default: return v;
  }
}

template <int AM, int BMD>
struct BGemm : BGemmArgs {
  static constexpr int AMODE = AM, BMODE = BMD;
  static constexpr bool QUAD_A = AM == BM_RK, QUAD_B = BMD == BM_RK;
  static constexpr int LA = AM == BM_RK ? RK_VEC : (AM == BM_KR ? KR_VEC : RK_GATHER);
  static constexpr int LB = BMD == BM_RK ? RK_VEC : (BMD == BM_KR ? KR_VEC : RK_GATHER);
  __host__ __device__ __forceinline__ int M() const { return m; }
  __host__ __device__ __forceinline__ int N() const { return n; }
  __host__ __device__ __forceinline__ int R() const { return r; }
  struct State {
    rsrc_t ra, rb;
    int arow, brow;
  };
  // one operand (rows = m or n) of a 64 x 32 tile, in the layout its mode stashes
  template <int MODE>
  __device__ __forceinline__ static void load_op(rsrc_t rs, int base_row, int rows, int r0, int R, int64_t s_row, int64_t s_r,
                                 float (&v)[8]) {
    const int tid = threadIdx.x;
    if constexpr (MODE == BM_RK) {  // rows tid/8 + 32 i, k = r0 + 4 (tid % 8) .. +3
      const int kk = r0 + 4 * (tid % 8);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = base_row + tid / 8 + 32 * i;
        const bool ok = (row < rows) & (kk < R);
        const unsigned addr = (unsigned)((row * s_row + kk) * 4);
        const f32x4 q = ld4(rs, ok ? addr : SENT, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * i + e] = q[e];
      }
    } else if constexpr (MODE == BM_KR) {  // rows 4 (tid % 16) .. +3, k = r0 + tid/16 + 16 i
      const int row = base_row + 4 * (tid % 16);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kk = r0 + tid / 16 + 16 * i;
        const bool ok = (row < rows) & (kk < R);
        const unsigned addr = (unsigned)((kk * s_r + row) * 4);
        const f32x4 q = ld4(rs, ok ? addr : SENT, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * i + e] = q[e];
      }
    } else {  // rows tid/32 + 8 i, k = r0 + tid % 32
      const int kk = r0 + tid % 32;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = base_row + tid / 32 + 8 * i;
        const bool ok = (row < rows) & (kk < R);
        const unsigned addr = (unsigned)((row * s_row + kk * s_r) * 4);
        v[i] = ld1(rs, ok ? addr : SENT, 0);
      }
    }
  }
  __device__ __forceinline__ State init(int k, int m0, int n0, int) const {
    State s;
    s.ra = make_rsrc(a + k * a_k, a_ext);
    s.rb = make_rsrc(b + k * b_k, b_ext);
    s.arow = m0;
    s.brow = n0;
    return s;
  }
  __device__ __forceinline__ void load_a(const State& s, int r0, float (&v)[8]) const {
    load_op<AM>(s.ra, s.arow, m, r0, r, a_m, a_r, v);
  }
  __device__ __forceinline__ void load_b(const State& s, int r0, float (&v)[8]) const {
    load_op<BMD>(s.rb, s.brow, n, r0, r, b_n, b_r, v);
  }
  __device__ __forceinline__ void store(int k, int mm, int nn, float v) const {
    const int64_t i = k * c_k + mm * c_m + nn * c_n;
    if (bias) v = bias[k * bias_k + nn] + v;
    if (add) v = add[i] + v;
    if (pre) pre[i] = v;
    if (act) v = apply_act(act, v, aux, i);
    if (mul) v = v * mul[i];
    c[i] = v;
  }
  // The S == 1 epilogue of one 32 x 32 accumulator tile (lane column n, rows
  // m[e]): every epilogue operand of the lane's 16 values is loaded before the
  // first store.  Per value, store()'s load -> store chain serialised on memory
  // latency (the stores may alias the operands): the bias epilogue cost 141 us
  // of 252 on the GRU input projection.  Same operations in the same order.
  __device__ __forceinline__ void store_tile(int k, int tm0, int tn0, int ml0, int nl, const f32x16& acc, int M,
                                             int N) const {
    // the plain epilogue's addressing: one uniform tile base, per value the
    // offset ml c_m + nl c_n (ml = ml0 + r, r = (e & 3) + 8 (e >> 2)), bounds as
    // predicates (no early exit)
    const int64_t tb = k * c_k + (int64_t)tm0 * c_m + (int64_t)tn0 * c_n;
    const bool nok = tn0 + nl < N;
    const float bv = (bias && nok) ? bias[k * bias_k + tn0 + nl] : 0.f;
    const bool use_aux = act >= FLR_ACT_DRELU && aux;
    float av[16], xv[16], mv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ml = ml0 + (e & 3) + 8 * (e >> 2);
      const bool ok = nok && tm0 + ml < M;
      const int64_t o = tb + ml * c_m + nl * c_n;
      av[e] = (add && ok) ? add[o] : 0.f;
      xv[e] = (use_aux && ok) ? aux[o] : 0.f;
      mv[e] = (mul && ok) ? mul[o] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ml = ml0 + (e & 3) + 8 * (e >> 2);
      if (nok && tm0 + ml < M) {
        const int64_t o = tb + ml * c_m + nl * c_n;
        float v = acc[e];
        if (bias) v = bv + v;
        if (add) v = av[e] + v;
        if (pre) pre[o] = v;
        if (act) v = apply_act_v(act, v, xv[e]);
        if (mul) v = v * mv[e];
        c[o] = v;
      }
    }
  }
  // the plain epilogue (row-major output, at most a bias: added there as bias + v)
  __device__ __forceinline__ bool linear() const { return c_n == 1 && !add && !act && !mul && !pre; }
  __device__ __forceinline__ float* out() const { return c; }
  __device__ __forceinline__ int64_t tile_base(int k, int m0, int n0) const { return k * c_k + m0 * c_m + n0; }
  __device__ __forceinline__ int64_t ldm() const { return c_m; }
  using State8 = State;
  template <int MODE>
  __device__ __forceinline__ static void load_op8(rsrc_t rs, int base_row, int rows, int r0, int R, int64_t s_row, int64_t s_r,
                                  float (&v)[8]) {
    const int tid = threadIdx.x;
    constexpr bool Q = MODE == BM_RK;
    const int row = base_row + stash_row<Q>(tid), kk0 = r0 + stash_k<Q>(tid);
    const bool rok = row < rows;
    if constexpr (MODE == BM_RK) {  // r contiguous, R % 4 == 0
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = rok & (kk0 + 4 * i < R);
        const unsigned addr = (unsigned)((row * s_row + kk0 + 4 * i) * 4);
        const f32x4 q = ld4(rs, ok ? addr : SENT, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * i + e] = q[e];
      }
    } else {  // KR (rows contiguous: lanes coalesce) and G
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool ok = rok & (kk0 + e < R);
        const unsigned addr = (unsigned)((row * s_row + (kk0 + e) * s_r) * 4);
        v[e] = ld1(rs, ok ? addr : SENT, 0);
      }
    }
  }
  __device__ __forceinline__ State8 init8(int k, int m0, int n0, int tid) const { return init(k, m0, n0, tid); }
  __device__ __forceinline__ void load_a8(const State8& s, int r0, float (&v)[8]) const {
    load_op8<AM>(s.ra, s.arow, m, r0, r, a_m, a_r, v);
  }
  __device__ __forceinline__ void load_b8(const State8& s, int r0, float (&v)[8]) const {
    load_op8<BMD>(s.rb, s.brow, n, r0, r, b_n, b_r, v);
  }
  // transposed-image loads of a k-contiguous (RK) operand (wsgemm_kernel): thread t
  // reads k = r0 + (t & 31) of rows 8 (t >> 5) .. +7 — a half-wave covers 128 B of a row
  using StateT = State;
  __device__ __forceinline__ StateT initT(int k, int m0, int n0, int tid) const { return init(k, m0, n0, tid); }
  __device__ __forceinline__ static void load_opT(rsrc_t rs, int base_row, int rows, int r0, int R, int64_t s_row, float (&v)[8]) {
    const int kk = r0 + (int)(threadIdx.x & 31);
    const int row0 = base_row + 8 * (int)(threadIdx.x >> 5);
    const unsigned base = (unsigned)((row0 * s_row + kk) * 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool ok = (row0 + i < rows) & (kk < R);
      v[i] = ld1(rs, ok ? base + (unsigned)(i * s_row * 4) : SENT, 0);
    }
  }
  __device__ __forceinline__ void load_at8(const StateT& s, int r0, float (&v)[8]) const {
    load_opT(s.ra, s.arow, m, r0, r, a_m, v);
  }
  __device__ __forceinline__ void load_bt8(const StateT& s, int r0, float (&v)[8]) const {
    load_opT(s.rb, s.brow, n, r0, r, b_n, v);
  }
  // LDS-DMA fill of one 128-row x 32-k operand image (dsgemm_kernel): 16 pieces of
  // 1 KB, one buffer_load_dwordx4 ... lds each, pieces 4 wave .. 4 wave + 3 issued by
  // this wave.  The destination is lane-linear, so the images' swizzles are applied
  // to the SOURCE address (lane -> the logical chunk its physical slot holds):
  //   RK [128 rows][32 k]: physical 16-B chunk of (row, q) = q ^ ((row >> 1) & 7)
  //      (a ds_read_b128 group of 16 rows hits 16 distinct bank groups);
  //   KR [32 k][128 rows]: physical 4-row chunk of (k, c) = c ^ (8 ((k >> 3) & 1))
  //      (the two half-waves' ds_read_b32, k and k + 8, on disjoint bank halves).
  // Out-of-range rows / reductions read 0 (raw buffer bounds), as the register loads.
  template <int MODE>
  __device__ __forceinline__ static void dma_op(rsrc_t rs, float* img, int base_row, int rows, int r0, int R, int64_t s_row,
                                int64_t s_r, int wave, int lane) {
    static_assert(MODE == BM_RK || MODE == BM_KR, "LDS-DMA images hold RK or KR operands");
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = 4 * wave + i;  // wave-uniform: the LDS base goes to M0
      unsigned voff;
      if constexpr (MODE == BM_RK) {  // 8 rows x 128 B per piece
        const int rl = 8 * piece + (lane >> 3);
        const int q = (lane & 7) ^ ((rl >> 1) & 7);
        const int row = base_row + rl, kk = r0 + 4 * q;
        voff = ((row < rows) & (kk < R)) ? (unsigned)((row * s_row + kk) * 4) : SENT;
      } else {  // 2 k-rows x 512 B per piece
        const int kl = 2 * piece + (lane >> 5);
        const int q = (lane & 31) ^ (((kl >> 3) & 1) << 3);
        const int row = base_row + 4 * q, kk = r0 + kl;
        voff = ((row < rows) & (kk < R)) ? (unsigned)((kk * s_r + row) * 4) : SENT;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(img + piece * 256), 16,
                                               voff, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void dma_a(const State& s, float* img, int r0, int wave, int lane) const {
    dma_op<AM>(s.ra, img, s.arow, m, r0, r, a_m, a_r, wave, lane);
  }
  __device__ __forceinline__ void dma_b(const State& s, float* img, int r0, int wave, int lane) const {
    dma_op<BMD>(s.rb, img, s.brow, n, r0, r, b_n, b_r, wave, lane);
  }
};

}  // namespace convt
}  // namespace flr
