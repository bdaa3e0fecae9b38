// Tap-major GEMM engine, unit 5 of 5: the batched dense GEMM (BGemm plans)
// and the row sums.
#include "conv_t_launch.h"

using namespace flr;

namespace {
// operand mode from strides: RK (r contiguous) / KR (rows contiguous) / G
int bgemm_mode(const float* p, int64_t s_k, int64_t s_row, int64_t s_r, int64_t rows, int64_t R) {
  const bool al = (reinterpret_cast<uintptr_t>(p) & 15) == 0 && s_k % 4 == 0;
  if (s_r == 1 && al && s_row % 4 == 0 && R % 4 == 0) return convt::BM_RK;
  if (s_row == 1 && al && s_r % 4 == 0 && rows % 4 == 0) return convt::BM_KR;
  return convt::BM_G;
}
template <int AM, int BMD>
int bgemm_run(const convt::BGemmArgs& args, void* ws, size_t ws_bytes, hipStream_t st) {
  convt::BGemm<AM, BMD> pl;
  static_cast<convt::BGemmArgs&>(pl) = args;
  return convt::launch(pl, ws, ws_bytes, st, "batched gemm");
}
template <int AM>
int bgemm_b(int bm, const convt::BGemmArgs& args, void* ws, size_t wsb, hipStream_t st) {
  switch (bm) {
    case convt::BM_RK: return bgemm_run<AM, convt::BM_RK>(args, ws, wsb, st);
    case convt::BM_KR: return bgemm_run<AM, convt::BM_KR>(args, ws, wsb, st);
    default: return bgemm_run<AM, convt::BM_G>(args, ws, wsb, st);
  }
}
}  // namespace

extern "C" size_t flr_bgemm_workspace(int64_t batch, int64_t M, int64_t N, int64_t R) {
  if (batch < 1 || M < 1 || N < 1 || R < 0 || M > INT32_MAX || N > INT32_MAX || R > INT32_MAX) return 0;
  convt::BGemm<convt::BM_G, convt::BM_G> pl;  // sizes only: the operand modes do not enter
  pl.m = (int)M; pl.n = (int)N; pl.r = (int)R;
  // either tile shape's split count (sub-tile count 1 or 4)
  size_t n = convt::splits_bytes(pl.m, pl.n, pl.r, batch, convt::plan_min_kt(pl));
#ifdef FLR_ABLATION
  // the pre-split form's bf16 planes of both operands (128 x 128 tiles), before the partials
  if (convt::bgemm_presplit() && convt::plan_tile(pl) == 22)
    n += (convt::ps_plane_bytes(batch, M, R) + 255) / 256 * 256 + (convt::ps_plane_bytes(batch, N, R) + 255) / 256 * 256;
#endif
  return n;
}

extern "C" int flr_bgemm(const float* A, int64_t a_k, int64_t a_m, int64_t a_r, const float* B, int64_t b_k,
                         int64_t b_n, int64_t b_r, float* C, int64_t c_k, int64_t c_m, int64_t c_n, const float* bias,
                         int64_t bias_k, const float* add, int64_t batch, int64_t M, int64_t N, int64_t R, void* ws,
                         size_t ws_bytes, void* stream) {
  return flr_bgemm_ex(A, a_k, a_m, a_r, B, b_k, b_n, b_r, C, c_k, c_m, c_n, bias, bias_k, add, FLR_ACT_NONE, nullptr,
                      nullptr, nullptr, batch, M, N, R, ws, ws_bytes, stream);
}

extern "C" int flr_bgemm_ex(const float* A, int64_t a_k, int64_t a_m, int64_t a_r, const float* B, int64_t b_k,
                            int64_t b_n, int64_t b_r, float* C, int64_t c_k, int64_t c_m, int64_t c_n,
                            const float* bias, int64_t bias_k, const float* add, int act, const float* mul,
                            const float* aux, float* pre, int64_t batch, int64_t M, int64_t N, int64_t R, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!A || !B || !C || batch < 1 || batch > 65535 || M < 1 || N < 1 || R < 1) return FLR_ERR_ARG;
  if (act < FLR_ACT_NONE || act > FLR_ACT_DTANH) return FLR_ERR_ARG;
  if (act >= FLR_ACT_DRELU && !aux) return FLR_ERR_ARG;
  if (a_k < 0 || a_m < 0 || a_r < 0 || b_k < 0 || b_n < 0 || b_r < 0 || c_k < 0 || c_m < 0 || c_n < 0)
    return FLR_ERR_ARG;
  const int64_t a_ext = (M - 1) * a_m + (R - 1) * a_r + 1;
  const int64_t b_ext = (N - 1) * b_n + (R - 1) * b_r + 1;
  if (a_ext * 4 >= (int64_t(1) << 31) || b_ext * 4 >= (int64_t(1) << 31) || M * N >= (int64_t(1) << 31) ||
      R >= (int64_t(1) << 30))
    return FLR_ERR_UNSUPPORTED;
  convt::BGemmArgs p;
  p.g.Kc = (int)batch;
  p.m = (int)M; p.n = (int)N; p.r = (int)R;
  p.a = A; p.a_k = a_k; p.a_m = a_m; p.a_r = a_r; p.a_ext = a_ext;
  p.b = B; p.b_k = b_k; p.b_n = b_n; p.b_r = b_r; p.b_ext = b_ext;
  p.c = C; p.c_k = c_k; p.c_m = c_m; p.c_n = c_n;
  p.bias = bias; p.bias_k = bias_k; p.add = add;
  p.act = act; p.mul = mul; p.aux = aux; p.pre = pre;
  hipStream_t st = as_stream(stream);
  const int am = bgemm_mode(A, a_k, a_m, a_r, M, R), bm = bgemm_mode(B, b_k, b_n, b_r, N, R);
  switch (am) {
    case convt::BM_RK: return bgemm_b<convt::BM_RK>(bm, p, ws, ws_bytes, st);
    case convt::BM_KR: return bgemm_b<convt::BM_KR>(bm, p, ws, ws_bytes, st);
    default: return bgemm_b<convt::BM_G>(bm, p, ws, ws_bytes, st);
  }
}

namespace flr {
namespace convt {
// out[k][n] = sum_m X[k][m][n] (bias gradients of the batched GEMMs).  Eight
// interleaved accumulators (rows m = 8i + j go to accumulator j), combined in a
// fixed tree: deterministic, and eight independent load/add chains per lane
// instead of one M-long dependent chain.
__global__ void sum_rows_kernel(const float* __restrict__ x, int64_t x_k, int64_t x_m, int M, int N,
                                float* __restrict__ out, int64_t out_k) {
  const int k = blockIdx.y;
  const int nn = blockIdx.x * blockDim.x + threadIdx.x;
  if (nn >= N) return;
  const float* p = x + k * x_k + nn;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int mm = 0;
  for (; mm + 8 <= M; mm += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += p[(int64_t)(mm + j) * x_m];
  }
  for (int j = 0; mm < M; ++mm, ++j) a[j] += p[(int64_t)mm * x_m];
  out[k * out_k + nn] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// Long reductions (the encoders' bias gradients sum M = 2080 rows) are cut
// into fixed 256-row chunks: stage 1 sums each chunk with the 8-accumulator
// kernel into a partial row, stage 2 adds the partials in chunk order.  The
// chunking depends on M alone, so a client's sum never depends on the launch.
constexpr int SR_CHUNK = 256;
constexpr int SR_MAXCHUNK = 64;

__global__ void sum_rows_chunks_kernel(const float* __restrict__ x, int64_t x_k, int64_t x_m, int M, int N,
                                       float* __restrict__ part, int nch) {
  const int k = blockIdx.z, c = blockIdx.y;
  const int nn = blockIdx.x * blockDim.x + threadIdx.x;
  if (nn >= N) return;
  const int m0 = c * SR_CHUNK, m1 = min(M, m0 + SR_CHUNK);
  const float* p = x + k * x_k + (int64_t)m0 * x_m + nn;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int mm = 0;
  const int R = m1 - m0;
  for (; mm + 8 <= R; mm += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += p[(int64_t)(mm + j) * x_m];
  }
  for (int j = 0; mm < R; ++mm, ++j) a[j] += p[(int64_t)mm * x_m];
  part[((int64_t)k * nch + c) * N + nn] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

__global__ void sum_rows_finish_kernel(const float* __restrict__ part, int nch, int N, float* __restrict__ out,
                                       int64_t out_k) {
  const int k = blockIdx.y;
  const int nn = blockIdx.x * blockDim.x + threadIdx.x;
  if (nn >= N) return;
  const float* p = part + (int64_t)k * nch * N + nn;
  float s = p[0];
  for (int c = 1; c < nch; ++c) s += p[(int64_t)c * N];
  out[k * out_k + nn] = s;
}
}  // namespace convt
}  // namespace flr

extern "C" size_t flr_sum_rows_workspace(int64_t batch, int64_t M, int64_t N) {
  if (batch < 1 || M <= convt::SR_CHUNK || N < 1) return 0;
  const int64_t nch = std::min<int64_t>((M + convt::SR_CHUNK - 1) / convt::SR_CHUNK, convt::SR_MAXCHUNK);
  return align_up((size_t)batch * nch * N * sizeof(float), 256);
}

extern "C" int flr_sum_rows(const float* X, int64_t x_k, int64_t x_m, int64_t batch, int64_t M, int64_t N, float* out,
                            int64_t out_k, void* stream) {
  return flr_sum_rows_ex(X, x_k, x_m, batch, M, N, out, out_k, nullptr, 0, stream);
}

extern "C" int flr_sum_rows_ex(const float* X, int64_t x_k, int64_t x_m, int64_t batch, int64_t M, int64_t N,
                               float* out, int64_t out_k, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X || !out || batch < 1 || batch > 65535 || M < 0 || N < 1) return FLR_ERR_ARG;
  const size_t need = flr_sum_rows_workspace(batch, M, N);
  if (need == 0 || !workspace || workspace_bytes < need ||
      (M + convt::SR_CHUNK - 1) / convt::SR_CHUNK > convt::SR_MAXCHUNK) {
    hipLaunchKernelGGL(convt::sum_rows_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)batch), dim3(256), 0,
                       as_stream(stream), X, x_k, x_m, (int)M, (int)N, out, out_k);
    return launch_status("sum_rows");
  }
  const int nch = (int)((M + convt::SR_CHUNK - 1) / convt::SR_CHUNK);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(convt::sum_rows_chunks_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)nch, (unsigned)batch),
                     dim3(256), 0, st, X, x_k, x_m, (int)M, (int)N, part, nch);
  int rc = launch_status("sum_rows_chunks");
  if (rc != FLR_OK) return rc;
  hipLaunchKernelGGL(convt::sum_rows_finish_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)batch), dim3(256), 0,
                     st, part, nch, (int)N, out, out_k);
  return launch_status("sum_rows_finish");
}
