// tests/u0_host/exp_probe.hip — TEST INFRASTRUCTURE: the device library's exp and spicey_exp (tran_common.h) on the same
// doubles read from a file, compiled like kernels.hip.
//   exp_probe <in.bin: n doubles> <out.bin: n doubles of exp, then n doubles of spicey_exp>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../spicey_amd/csrc/tran_common.h"

__global__ void exp_kernel(const double *x, double *lib, double *port, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    lib[i] = exp(x[i]);
    port[i] = spicey_exp(x[i]);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> x;
  double buf;
  while (fread(&buf, sizeof(double), 1, f) == 1) x.push_back(buf);
  fclose(f);
  const long n = (long)x.size();
  if (n == 0) return 2;
  std::vector<double> out((size_t)n * 2);
  double *d_x = nullptr, *d_out = nullptr;
  if (hipMalloc((void **)&d_x, x.size() * sizeof(double)) != hipSuccess || hipMalloc((void **)&d_out, out.size() * sizeof(double)) != hipSuccess) return 3;
  if (hipMemcpy(d_x, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 3;
  hipLaunchKernelGGL(exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_x, d_out, d_out + n, n);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
  if (hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 3;
  (void)hipFree(d_x);
  (void)hipFree(d_out);
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out.data(), sizeof(double), out.size(), f);
  fclose(f);
  return 0;
}
