// spectrum.hip — the spectrum of a transient's waveforms on the device (spicey_spectrum_device): kernel and launcher.
//
// A pass of its own over the step-major buffers [inst][step][col] a transient kernel wrote; spectrum_exec.h holds the
// arithmetic and the thread mapping, shared with the CPU harness of tests/spectrum_host.  Unlike the streaming reductions
// of measure.hip, fourier.hip and timing.hip this is a batched FFT in LDS: one workgroup of 256 threads per (instance,
// request) item, items taken grid-stride.  The N samples are gathered from global memory straight into their bit-reversed
// slots of two planes re[N] | im[N] in dynamic LDS (16 N bytes: 128 KiB at N = 8192, so one workgroup per CU there and
// 160 KiB / 16 N of them below), the log2 N radix-2 stages run in place with a barrier between them — thread t takes the
// butterflies t, t + 256, ... of a stage, so neighbouring lanes read neighbouring twiddles and, from h = 32 on, each
// half-wave neighbouring slots — and the band or the dominant bin is written from the planes.  The twiddles and the window
// come from tables the host built (the device never evaluates a sine); they are read through the cache, not staged.  One
// launch per distinct N of the list, so a short transform does not pay for the LDS of a long one; no atomics, no waiting
// on other workgroups.
// Bit identity with the CPU harness needs every product and sum rounded on its own: no FMA contraction in this
// translation unit (as measure.hip).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <vector>

#include "devbuf.h"
#include "measure.h"
#include "spectrum.h"

namespace {

__global__ void __launch_bounds__(SPICEY_SPEC_THREADS) spicey_spectrum_kernel(int64_t items, int32_t count, int32_t n_req, int64_t n_points,
                                                                              const double *__restrict__ a_v, int32_t n_v, const double *__restrict__ a_i, int32_t n_i,
                                                                              const SpiceySpecDevReq *__restrict__ table, const int32_t *__restrict__ order,
                                                                              const double *__restrict__ tables, int32_t log2n, double *__restrict__ out,
                                                                              int32_t out_stride) {
  extern __shared__ double planes[];
  __shared__ double cand_p[SPICEY_SPEC_THREADS];
  __shared__ int32_t cand_k[SPICEY_SPEC_THREADS];
  double *re = planes, *im = planes + ((size_t)1 << log2n);
  const int32_t t = (int32_t)threadIdx.x;
  const auto par = [t](auto f) {
    f(t);
    __syncthreads();
  };
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t inst = item / count;
    const int32_t r = order[item - inst * count];
    const SpiceySpecDevReq q = table[r];
    const int64_t n = q.signal ? n_i : n_v;
    const double *base = (q.signal ? a_i : a_v) + inst * n_points * n;
    spicey_spec_item(par, SPICEY_SPEC_THREADS, q, tables, base, n, re, im, cand_p, cand_k, out + (inst * n_req + r) * out_stride, out_stride);
  }
}

}  // namespace

hipError_t spicey_launch_spectrum(int device, int32_t n_inst, int64_t n_points, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                  const SpiceySpecPlan &plan, double *d_out, int32_t out_stride, void *d_work, hipStream_t st) {
  hipError_t e;
  std::vector<unsigned char> head;
  spicey_spec_head(plan, head);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const char *w = (const char *)d_work;
  const SpiceySpecDevReq *d_table = (const SpiceySpecDevReq *)w;
  const int32_t *d_order = (const int32_t *)(w + plan.off_order);
  const double *d_tables = (const double *)(w + plan.off_tables);
  const int32_t n_req = (int32_t)plan.table.size();
  for (const SpiceySpecLaunch &L : plan.launches) {
    const size_t lds = spicey_spec_lds_bytes(L.log2n);
    if ((e = spicey_allow_dyn_lds(spicey_spectrum_kernel, lds)) != hipSuccess) return e;
    const int64_t items = (int64_t)n_inst * L.count;
    hipLaunchKernelGGL(spicey_spectrum_kernel, dim3(spicey_meas_grid1(items)), dim3(SPICEY_SPEC_THREADS), lds, st, items, L.count, n_req, n_points, d_v, n_v, d_i, n_i,
                       d_table, d_order + L.first, d_tables, L.log2n, d_out, out_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}
