// tests/ac_exact_host/hypot_probe.hip — TEST INFRASTRUCTURE: the device's spicey_v8_hypot (ac_exact_exec.h) on pairs read
// from a file, compiled like ac_exact.hip (no FMA contraction).
//   hypot_probe <in.bin: n x 2 doubles> <out.bin: n doubles>
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../spicey_amd/csrc/ac_exact_exec.h"

__global__ void hypot_kernel(const double *xy, double *out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = spicey_v8_hypot(xy[2 * i], xy[2 * i + 1]);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> xy;
  double buf[2];
  while (fread(buf, sizeof(double), 2, f) == 2) xy.insert(xy.end(), buf, buf + 2);
  fclose(f);
  const long n = (long)(xy.size() / 2);
  std::vector<double> out((size_t)n);
  double *d_xy = nullptr, *d_out = nullptr;
  if (hipMalloc((void **)&d_xy, xy.size() * sizeof(double) + 16) != hipSuccess || hipMalloc((void **)&d_out, out.size() * sizeof(double) + 16) != hipSuccess) return 3;
  if (hipMemcpy(d_xy, xy.data(), xy.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 3;
  hipLaunchKernelGGL(hypot_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_xy, d_out, n);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
  if (hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 3;
  (void)hipFree(d_xy);
  (void)hipFree(d_out);
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out.data(), sizeof(double), out.size(), f);
  fclose(f);
  return 0;
}
