// timing.hip — edge timing on the device (spicey_timing_device): kernels and launcher.
//
// A reduction pass of its own over the step-major buffers [inst][step][col] a transient kernel wrote; timing_exec.h holds
// the arithmetic and the mapping, shared with the CPU harness of tests/timing_host.  The base windows of relative levels
// run first, as stats requests through the kernels of measure.hip (spicey_launch_measure) into a region of this pass's
// workspace, on the same stream.  Then two kernels, no atomics, no waiting on other workgroups, no LDS:
//   stage 1  one thread per (instance, edge, chunk of SPICEY_MEAS_CHUNK intervals): the lanes of a wave take neighbouring
//            edges — the table is sorted by column, so a wave instruction reads neighbouring addresses of one row — and
//            with fewer edges than lanes the rest of the workgroup spreads over chunks.  Each thread resolves its
//            instance's level from the base rows, walks its chunk in step order and leaves one int32 count.
//   stage 2  one thread per (instance, request) adds the counts in ascending chunk order, walks the one chunk that holds
//            the wanted crossing again and writes the row of the result the caller's list names (the serial form of the
//            selection; threads are ordered by their targ's column, so the second walk is coalesced only as far as
//            neighbouring requests want the same chunk of neighbouring columns).
// Bit identity with the CPU harness needs every product and sum rounded on its own: no FMA contraction in this
// translation unit (as measure.hip).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <vector>

#include "measure.h"
#include "timing.h"
#include "timing_exec.h"

namespace {

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_timing_stage1(int32_t n_inst, int64_t n_points, const double *__restrict__ a_v, int32_t n_v,
                                                                            const double *__restrict__ a_i, int32_t n_i,
                                                                            const SpiceyTimDevEdge *__restrict__ edges, int32_t n_edge, int32_t n_base,
                                                                            const double *__restrict__ base_out, int32_t *__restrict__ counts) {
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_edge, SPICEY_MEAS_THREADS);
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x)
    spicey_tim_stage1(g, tile, (int32_t)threadIdx.x, edges, n_edge, n_base, n_points, a_v, n_v, a_i, n_i, base_out, counts);
}

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_timing_stage2(int64_t total, const SpiceyTimDevReq *__restrict__ reqs, int32_t n_req,
                                                                            const SpiceyTimDevEdge *__restrict__ edges, int32_t n_edge, int32_t n_base,
                                                                            int64_t max_chunks, int64_t n_points, double dt, const double *__restrict__ a_v,
                                                                            int32_t n_v, const double *__restrict__ a_i, int32_t n_i,
                                                                            const double *__restrict__ base_out, const int32_t *__restrict__ counts,
                                                                            double *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MEAS_THREADS + threadIdx.x;
  if (idx < total) spicey_tim_stage2(idx, reqs, n_req, edges, n_edge, n_base, max_chunks, n_points, dt, a_v, n_v, a_i, n_i, base_out, counts, out);
}

}  // namespace

hipError_t spicey_launch_timing(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                const SpiceyTimPlan &plan, double *d_out, void *d_work, hipStream_t st) {
  hipError_t e;
  std::vector<unsigned char> head;
  spicey_tim_head(plan, head);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  char *w = (char *)d_work;
  const SpiceyTimDevEdge *d_edges = (const SpiceyTimDevEdge *)w;
  const SpiceyTimDevReq *d_reqs = (const SpiceyTimDevReq *)(w + plan.off_reqs);
  double *d_base = (double *)(w + plan.off_base_out());
  int32_t *d_counts = (int32_t *)(w + plan.off_counts(n_inst, n_points));
  const int32_t n_edge = (int32_t)plan.edges.size(), n_req = (int32_t)plan.reqs.size(), n_base = (int32_t)plan.bases.size();
  if (n_base > 0 &&
      (e = spicey_launch_measure(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan.bases.data(), n_base, d_base, w + plan.off_base_work(n_inst), st)) != hipSuccess)
    return e;
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_edge, SPICEY_MEAS_THREADS);
  hipLaunchKernelGGL(spicey_timing_stage1, dim3(spicey_meas_grid1(g.tiles)), dim3(SPICEY_MEAS_THREADS), 0, st, n_inst, n_points, d_v, n_v, d_i, n_i, d_edges, n_edge, n_base,
                     (const double *)d_base, d_counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t total = (int64_t)n_inst * n_req;
  unsigned grid2 = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MEAS_THREADS, &grid2)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_timing_stage2, dim3(grid2), dim3(SPICEY_MEAS_THREADS), 0, st, total, d_reqs, n_req, d_edges, n_edge, n_base, plan.max_chunks,
                     n_points, dt, d_v, n_v, d_i, n_i, (const double *)d_base, (const int32_t *)d_counts, d_out);
  return hipGetLastError();
}
