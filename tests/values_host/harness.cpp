// CPU harness of the values pass: values_exec.h — the code the kernels of spicey_amd/csrc/values.hip run — through an
// emulation of their lane and item mapping: the rows are cleared; workgroups of `threads` threads take the trace stage 1
// tiles blockIdx, blockIdx + grid, ..., every thread of a workgroup does what spicey_val_stage1 gives it; then one thread
// per (instance, trace request, bucket) combines (spicey_val_stage2) and one per (instance, point) interpolates
// (spicey_val_points).  The call is judged by spicey_val_judge of values.h, the judge of the library's entry points, and
// the tables are read from the head block spicey_val_head builds, at the offsets the launcher uses.  Compiled with
// -ffp-contract=off like the kernels' translation unit, so the results are the GPU's bit for bit.  The partials start as
// NaNs: one that is read without having been written shows.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/values.h"

extern "C" int32_t spicey_values_host_chunk(void) { return SPICEY_MEAS_CHUNK; }
extern "C" int32_t spicey_values_host_threads(void) { return SPICEY_MEAS_THREADS; }
extern "C" int32_t spicey_values_host_max_buckets(void) { return SPICEY_TRACE_MAX_BUCKETS; }
extern "C" int64_t spicey_values_host_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyValReq *reqs, int32_t n_req, int64_t n_pts) {
  return spicey_val_workspace_bytes(n_inst, n_points, reqs, n_req, n_pts);
}

// threads: a power of two, 1 .. 1024; grid: workgroups launched, 0 = one per tile.  have_out = 0 stands for null result or
// workspace buffers, work_bytes = -1 for a workspace of exactly the size needed.  timing: [n_inst][n_timing][8] or null.
// Returns SPICEY_OK or SPICEY_ERR_BAD_DESC (text in err; `rows` untouched).
extern "C" int32_t spicey_values_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                          const SpiceyValReq *reqs, int32_t n_req, const SpiceyValPoint *pts, int64_t n_pts, const double *timing,
                                          int32_t n_timing, double *rows, int32_t out_stride, int32_t have_out, int64_t work_bytes, int32_t threads, int64_t grid,
                                          char *err, int32_t err_cap) {
  std::string e;
  SpiceyValPlan plan;
  bool ok = threads >= 1 && threads <= 1024 && (threads & (threads - 1)) == 0 && grid >= 0;
  if (!ok) e = "values: bad arguments of the emulated launch";
  const int64_t need = spicey_val_workspace_bytes(n_inst, n_points, reqs, n_req, n_pts);
  ok = ok && spicey_val_judge(n_inst, n_points, dt, v != nullptr, n_v, i != nullptr, n_i, reqs, n_req, pts, n_pts, timing != nullptr, n_timing, have_out != 0 && rows,
                              out_stride, work_bytes < 0 ? need : work_bytes, plan, e);
  if (!ok) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  std::vector<unsigned char> head;
  spicey_val_head(plan, pts, head);
  const SpiceyValPoint *h_pts = (const SpiceyValPoint *)head.data();
  const SpiceyValDevTrace *traces = (const SpiceyValDevTrace *)(head.data() + plan.off_traces);
  const SpiceyValDevPts *points = (const SpiceyValDevPts *)(head.data() + plan.off_points);
  std::vector<double> partials((size_t)(plan.workspace_bytes(n_inst) - plan.head_bytes) / sizeof(double), std::numeric_limits<double>::quiet_NaN());
  for (int64_t k = 0; k < (int64_t)n_inst * n_req * out_stride; k++) rows[k] = 0.0;
  const int32_t n_trace = (int32_t)plan.traces.size();
  if (n_trace > 0) {
    const SpiceyMeasGeom g = spicey_val_geom(n_inst, plan.max_items, n_trace, threads);
    const int64_t blocks = grid == 0 || grid > g.tiles ? g.tiles : grid;
    for (int64_t b = 0; b < blocks; b++)
      for (int64_t tile = b; tile < g.tiles; tile += blocks)
        for (int32_t t = 0; t < threads; t++)
          spicey_val_stage1(g, tile, t, traces, n_trace, plan.total_items, n_points, v, n_v, i, n_i, partials.data());
    for (int64_t idx = 0; idx < (int64_t)n_inst * n_trace * plan.max_B; idx++)
      spicey_val_stage2(idx, traces, n_trace, plan.max_B, plan.total_items, n_req, partials.data(), rows, out_stride);
  }
  for (int64_t idx = 0; idx < (int64_t)n_inst * plan.total_pitems; idx++)
    spicey_val_points(idx, points, (int32_t)plan.points.size(), plan.total_pitems, h_pts, timing, n_timing, n_points, dt, v, n_v, i, n_i, n_req, rows, out_stride);
  return SPICEY_OK;
}
