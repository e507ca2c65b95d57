// fourier.hip — harmonics of a transient's waveforms on the device (spicey_fourier_device): kernels and launcher.
//
// A reduction pass of its own over the step-major buffers [inst][step][col] a transient kernel wrote; fourier_exec.h holds
// the arithmetic and the mapping, shared with the CPU harness of tests/fourier_host.  Two kernels, no atomics, no waiting
// on other workgroups:
//   stage 1  one thread per (request, chunk of SPICEY_MEAS_CHUNK steps).  The 64 lanes of a wave take neighbouring requests
//            of ONE basis (f0, window) — the table is sorted by (basis, signal, column), so a wave instruction reads
//            neighbouring addresses of one row — and the four waves of a workgroup take four chunks.  A wave is thus at one
//            step of one twiddle table at a time: the chunk index comes through readfirstlane, so the compiler sees the
//            twiddle address as wave-uniform and fetches the table with scalar loads (no LDS staging, no barrier; the 64 KB
//            a chunk's table may take would otherwise cap a CU at two workgroups).  The sample is loaded once per step and
//            meets all 2 H twiddles of that step; the 1 + 2 H running sums live in registers (one instance of the loop per
//            H, switch on the basis' H).
//   stage 2  one thread per (instance, request, element of the caller's row) adds that element's chunk partials in
//            ascending chunk order; elements past the request's 1 + 2 n_harm are written as 0.
// Bit identity with the CPU harness needs every product and sum rounded on its own: no FMA contraction in this
// translation unit (as measure.hip).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <vector>

#include "fourier.h"
#include "fourier_exec.h"
#include "measure.h"

namespace {

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_fourier_stage1(int64_t tiles, int64_t tiles_per_inst, int64_t n_points,
                                                                             const double *__restrict__ a_v, int32_t n_v, const double *__restrict__ a_i, int32_t n_i,
                                                                             const SpiceyFourDevReq *__restrict__ table, const SpiceyFourBasis *__restrict__ bases,
                                                                             int32_t n_basis, const double *__restrict__ tw, double *__restrict__ partials,
                                                                             int64_t partials_per_inst) {
  const int32_t lane = (int32_t)(threadIdx.x % SPICEY_FOUR_WAVE);
  const int32_t slot = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x / SPICEY_FOUR_WAVE));
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    spicey_four_stage1(tile, lane, slot, SPICEY_FOUR_WAVE, SPICEY_MEAS_THREADS / SPICEY_FOUR_WAVE, tiles_per_inst, table, bases, n_basis, tw, n_points, a_v, n_v,
                       a_i, n_i, partials, partials_per_inst);
}

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_fourier_stage2(int64_t total, const SpiceyFourDevReq *__restrict__ table,
                                                                             const SpiceyFourBasis *__restrict__ bases, int32_t n_req, int32_t out_stride,
                                                                             const double *__restrict__ partials, int64_t partials_per_inst,
                                                                             double *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MEAS_THREADS + threadIdx.x;
  if (idx < total) spicey_four_stage2(idx, table, bases, n_req, out_stride, partials, partials_per_inst, out);
}

}  // namespace

hipError_t spicey_launch_fourier(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                 const SpiceyFourPlan &plan, double *d_out, int32_t out_stride, void *d_work, hipStream_t st) {
  hipError_t e;
  std::vector<unsigned char> head;
  spicey_four_head(plan, dt, head);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const char *w = (const char *)d_work;
  const SpiceyFourDevReq *d_table = (const SpiceyFourDevReq *)w;
  const SpiceyFourBasis *d_bases = (const SpiceyFourBasis *)(w + plan.off_bases);
  const double *d_tw = (const double *)(w + plan.off_tw);
  double *partials = (double *)((char *)d_work + plan.head_bytes);
  const int32_t n_req = (int32_t)plan.table.size();
  const int64_t tiles = (int64_t)n_inst * plan.tiles_per_inst;
  hipLaunchKernelGGL(spicey_fourier_stage1, dim3(spicey_meas_grid1(tiles)), dim3(SPICEY_MEAS_THREADS), 0, st, tiles, plan.tiles_per_inst, n_points, d_v, n_v, d_i, n_i, d_table, d_bases,
                     (int32_t)plan.bases.size(), d_tw, partials, plan.partials_per_inst);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t total = (int64_t)n_inst * n_req * out_stride;
  unsigned grid2 = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MEAS_THREADS, &grid2)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_fourier_stage2, dim3(grid2), dim3(SPICEY_MEAS_THREADS), 0, st, total, d_table, d_bases, n_req, out_stride,
                     (const double *)partials, plan.partials_per_inst, d_out);
  return hipGetLastError();
}
