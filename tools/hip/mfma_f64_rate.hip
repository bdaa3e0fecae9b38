// Microbenchmark: the issue rate of v_mfma_f64_16x16x4_f64, the instruction of
// flr_rows_gram (agg_foolsgold.hip), from a register-only loop: ACC independent
// accumulators per wave (the Gram kernel holds 4), one or two waves per SIMD on
// every SIMD of the device.  Prints the device-wide MFMA rate, the fp64 FLOP/s
// it stands for (2 * 16 * 16 * 4 per instruction) and the SIMD cycles per
// instruction at a nominal 2.4 GHz.  Timing only: operands are constants.
// Build: hipcc -O3 --offload-arch=gfx950 mfma_f64_rate.hip -o mfma_f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int ACC>
__global__ __launch_bounds__(256) void k(const double* in, double* out, int iters) {
  const double a = in[threadIdx.x & 63], b = in[(threadIdx.x + 1) & 63];
  f64x4 acc[ACC];
#pragma unroll
  for (int i = 0; i < ACC; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 16 / ACC; ++r) {
#pragma unroll
      for (int i = 0; i < ACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
  }
  double r = 0.0;
#pragma unroll
  for (int i = 0; i < ACC; ++i) r += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

template <int ACC>
void run(int cus, int wps, double* in, double* out) {
  const int iters = 16384;  // 16 MFMAs per trip
  const dim3 grid(cus * wps), block(256);  // 4 waves per workgroup: one per SIMD
  hipLaunchKernelGGL((k<ACC>), grid, block, 0, 0, in, out, iters);
  (void)hipDeviceSynchronize();
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a);
  hipLaunchKernelGGL((k<ACC>), grid, block, 0, 0, in, out, iters);
  (void)hipEventRecord(b);
  (void)hipEventSynchronize(b);
  float ms;
  (void)hipEventElapsedTime(&ms, a, b);
  const double per_simd = (double)iters * 16 * wps;        // instructions one SIMD issued
  const double total = per_simd * 4.0 * cus;
  printf("{\"accumulators\": %d, \"waves_per_simd\": %d, \"ms\": %.3f, \"mfma_per_s\": %.4g, \"fp64_tflops\": %.2f, "
         "\"simd_cycles_per_mfma_at_2.4GHz\": %.2f}\n",
         ACC, wps, ms, total / (ms * 1e-3), total * 2048.0 / (ms * 1e-3) / 1e12, ms * 1e-3 * 2.4e9 / per_simd);
}

int main() {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) {
    printf("no device\n");
    return 1;
  }
  const int cus = prop.multiProcessorCount;
  printf("{\"device\": \"%s\", \"compute_units\": %d}\n", prop.gcnArchName, cus);
  double *in, *out;
  (void)hipMalloc(&in, 64 * sizeof(double));
  (void)hipMalloc(&out, (size_t)cus * 2 * 256 * sizeof(double));
  (void)hipMemset(in, 0, 64 * sizeof(double));
  for (int wps : {1, 2}) {
    run<1>(cus, wps, in, out);
    run<4>(cus, wps, in, out);
    run<8>(cus, wps, in, out);
  }
  return 0;
}
