// power.hip — products of two signals reduced on the device (spicey_power_device): kernels and launcher.
//
// A reduction pass of its own over the step-major buffers [inst][step][col] a transient kernel wrote; power_exec.h holds
// the arithmetic and the mapping, shared with the CPU harness of tests/power_host.  Two kernels, no LDS, no barrier, no
// atomics, no waiting on other workgroups:
//   stage 1  one thread per (request, chunk of SPICEY_MEAS_CHUNK steps), the mapping of measure.hip: the lanes of a wave
//            take neighbouring requests of the table sorted by (a_signal, a_col, b_signal, b_col), so a wave instruction
//            reads neighbouring columns of one row, and with fewer requests than lanes the rest of the workgroup spreads
//            over chunks.  Each thread walks its chunk in step order — two to four strided 8-byte loads per step, several
//            steps' loads in flight (SPICEY_MEAS_UNROLL), its 13 running values in registers — and leaves them in the
//            workspace.
//   stage 2  one thread per (instance, request) combines the request's chunk partials in ascending chunk order and writes
//            the row of the result the caller's list names, tail zeros included.
// Bit identity with the CPU harness needs every product and sum rounded on its own: no FMA contraction in this
// translation unit (as measure.hip).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "measure.h"
#include "power.h"

namespace {

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_power_stage1_kernel(int32_t n_inst, int64_t n_points, const double *__restrict__ a_v, int32_t n_v,
                                                                                  const double *__restrict__ a_i, int32_t n_i,
                                                                                  const SpiceyPowerDevReq *__restrict__ table, int32_t n_req,
                                                                                  double *__restrict__ partials) {
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_req, SPICEY_MEAS_THREADS);
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x)
    spicey_power_stage1(g, tile, (int32_t)threadIdx.x, table, n_req, n_points, a_v, n_v, a_i, n_i, partials);
}

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_power_stage2_kernel(int64_t total, const SpiceyPowerDevReq *__restrict__ table, int32_t n_req,
                                                                                  int64_t max_chunks, const double *__restrict__ partials,
                                                                                  double *__restrict__ rows) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MEAS_THREADS + threadIdx.x;
  if (idx < total) spicey_power_stage2(idx, table, n_req, max_chunks, partials, rows);
}

}  // namespace

hipError_t spicey_launch_power(int device, int32_t n_inst, int64_t n_points, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                               const SpiceyPowerDevReq *table, int32_t n_req, double *d_out, void *d_work, hipStream_t st) {
  hipError_t e;
  if ((e = spicey_upload_table_async(device, d_work, table, (size_t)n_req * sizeof(SpiceyPowerDevReq), st)) != hipSuccess) return e;
  const SpiceyPowerDevReq *d_table = (const SpiceyPowerDevReq *)d_work;
  double *partials = (double *)((char *)d_work + spicey_power_head_bytes(n_req));
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_req, SPICEY_MEAS_THREADS);
  hipLaunchKernelGGL(spicey_power_stage1_kernel, dim3(spicey_meas_grid1(g.tiles)), dim3(SPICEY_MEAS_THREADS), 0, st, n_inst, n_points, d_v, n_v, d_i, n_i, d_table,
                     n_req, partials);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t total = (int64_t)n_inst * n_req;
  unsigned grid2 = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MEAS_THREADS, &grid2)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_power_stage2_kernel, dim3(grid2), dim3(SPICEY_MEAS_THREADS), 0, st, total, d_table, n_req, g.max_chunks, (const double *)partials, d_out);
  return hipGetLastError();
}
