// values.hip — waveform values reduced on the device (spicey_values_device): kernels and launcher.
//
// A pass of its own over the step-major buffers [inst][step][col] a transient kernel wrote; values_exec.h holds the
// arithmetic and the mapping, shared with the CPU harness of tests/values_host.  Three kernels, no LDS, no barrier, no
// atomics, no waiting on other workgroups:
//   trace stage 1  one thread per (trace request, bucket, sub-chunk of SPICEY_MEAS_CHUNK steps), the geometry of measure.hip
//                  with a request's B * S items in the place of chunks: the lanes of a wave take neighbouring requests of
//                  the table sorted by (signal, window, B, col), so a wave instruction reads neighbouring columns of one row
//                  where the list allows, and with fewer requests than lanes the rest of the workgroup spreads over items.
//                  Each thread walks its own sub-chunk in step order — one or two strided 8-byte loads per step, several
//                  steps' loads in flight (SPICEY_MEAS_UNROLL) — and leaves {min, step, max, step, first, last} in the
//                  workspace; a bucket that ends early ends only that thread's loop.
//   trace stage 2  one thread per (instance, trace request, bucket) combines the bucket's sub-chunk partials in ascending
//                  order and writes the bucket's 6 doubles into the row the caller's list names.
//   points         one thread per (instance, point of a POINTS run | FIND request): two to four loads, one interpolation.
// The rows are cleared first (hipMemsetAsync), so the doubles behind a request's own are 0.
// Bit identity with the CPU harness needs every product and sum rounded on its own: no FMA contraction in this
// translation unit (as measure.hip).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <vector>

#include "measure.h"
#include "values.h"

namespace {

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_values_stage1_kernel(int32_t n_inst, int64_t n_points, const double *__restrict__ a_v, int32_t n_v,
                                                                                   const double *__restrict__ a_i, int32_t n_i,
                                                                                   const SpiceyValDevTrace *__restrict__ table, int32_t n_trace, int64_t max_items,
                                                                                   int64_t total_items, double *__restrict__ partials) {
  const SpiceyMeasGeom g = spicey_val_geom(n_inst, max_items, n_trace, SPICEY_MEAS_THREADS);
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x)
    spicey_val_stage1(g, tile, (int32_t)threadIdx.x, table, n_trace, total_items, n_points, a_v, n_v, a_i, n_i, partials);
}

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_values_stage2_kernel(int64_t total, const SpiceyValDevTrace *__restrict__ table, int32_t n_trace,
                                                                                   int32_t max_B, int64_t total_items, int32_t n_req,
                                                                                   const double *__restrict__ partials, double *__restrict__ rows,
                                                                                   int32_t out_stride) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MEAS_THREADS + threadIdx.x;
  if (idx < total) spicey_val_stage2(idx, table, n_trace, max_B, total_items, n_req, partials, rows, out_stride);
}

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_values_points_kernel(int64_t total, const SpiceyValDevPts *__restrict__ table, int32_t n_preq,
                                                                                   int64_t total_pitems, const SpiceyValPoint *__restrict__ pts,
                                                                                   const double *__restrict__ timing, int32_t n_timing, int64_t n_points, double dt,
                                                                                   const double *__restrict__ a_v, int32_t n_v, const double *__restrict__ a_i,
                                                                                   int32_t n_i, int32_t n_req, double *__restrict__ rows, int32_t out_stride) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MEAS_THREADS + threadIdx.x;
  if (idx < total) spicey_val_points(idx, table, n_preq, total_pitems, pts, timing, n_timing, n_points, dt, a_v, n_v, a_i, n_i, n_req, rows, out_stride);
}

}  // namespace

hipError_t spicey_launch_values(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                const SpiceyValPlan &plan, const SpiceyValPoint *pts, const double *d_timing, int32_t n_timing, double *d_out, int32_t out_stride,
                                void *d_work, hipStream_t st) {
  hipError_t e;
  std::vector<unsigned char> head;
  spicey_val_head(plan, pts, head);
  if (!head.empty() && (e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(d_out, 0, (size_t)n_inst * (size_t)plan.n_req * (size_t)out_stride * sizeof(double), st)) != hipSuccess) return e;
  const char *w = (const char *)d_work;
  const SpiceyValPoint *d_pts = (const SpiceyValPoint *)w;
  const SpiceyValDevTrace *d_traces = (const SpiceyValDevTrace *)(w + plan.off_traces);
  const SpiceyValDevPts *d_points = (const SpiceyValDevPts *)(w + plan.off_points);
  double *partials = (double *)((char *)d_work + plan.head_bytes);
  unsigned grid = 0;
  if (!plan.traces.empty()) {
    const int32_t n_trace = (int32_t)plan.traces.size();
    const SpiceyMeasGeom g = spicey_val_geom(n_inst, plan.max_items, n_trace, SPICEY_MEAS_THREADS);
    hipLaunchKernelGGL(spicey_values_stage1_kernel, dim3(spicey_meas_grid1(g.tiles)), dim3(SPICEY_MEAS_THREADS), 0, st, n_inst, n_points, d_v, n_v, d_i, n_i, d_traces,
                       n_trace, plan.max_items, plan.total_items, partials);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t total = (int64_t)n_inst * n_trace * plan.max_B;
    if ((e = spicey_meas_grid2(total, SPICEY_MEAS_THREADS, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(spicey_values_stage2_kernel, dim3(grid), dim3(SPICEY_MEAS_THREADS), 0, st, total, d_traces, n_trace, plan.max_B, plan.total_items, plan.n_req,
                       (const double *)partials, d_out, out_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!plan.points.empty()) {
    const int64_t total = (int64_t)n_inst * plan.total_pitems;
    if ((e = spicey_meas_grid2(total, SPICEY_MEAS_THREADS, &grid)) != hipSuccess) return e;
    hipLaunchKernelGGL(spicey_values_points_kernel, dim3(grid), dim3(SPICEY_MEAS_THREADS), 0, st, total, d_points, (int32_t)plan.points.size(), plan.total_pitems, d_pts,
                       d_timing, n_timing, n_points, dt, d_v, n_v, d_i, n_i, plan.n_req, d_out, out_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}
