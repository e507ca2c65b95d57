// CPU harness of the edge-timing pass: timing_exec.h — the code the kernels of spicey_amd/csrc/timing.hip run — through an
// emulation of their lane and chunk mapping.  The base windows go through the measurement pass's own stage 1 / stage 2
// (measure_exec.h) into the base rows, as on the device; then workgroups of `threads` threads take the stage 1 tiles
// blockIdx, blockIdx + grid, ..., every thread of a workgroup does what spicey_tim_stage1 gives it, and one thread per
// (instance, request) selects (spicey_tim_stage2).  Compiled with -ffp-contract=off like the kernels' translation unit, so
// the results are the GPU's bit for bit.  Base rows start as NaNs and counts as a negative pattern: one that is read
// without having been written shows.
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/timing_exec.h"

extern "C" int32_t spicey_tim_host_chunk(void) { return SPICEY_MEAS_CHUNK; }
extern "C" int32_t spicey_tim_host_threads(void) { return SPICEY_MEAS_THREADS; }
extern "C" int64_t spicey_tim_host_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyTimingReq *reqs, int32_t n_req) {
  return spicey_tim_workspace_bytes(n_inst, n_points, reqs, n_req);
}

// threads: a power of two, 1 .. 1024; grid: workgroups launched, 0 = one per tile; work_bytes: what the caller claims its
// workspace holds (-1: exactly enough).  Returns SPICEY_OK or SPICEY_ERR_BAD_DESC (text in err; `out` untouched).
extern "C" int32_t spicey_tim_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                       const SpiceyTimingReq *reqs, int32_t n_req, double *out, int64_t work_bytes, int32_t threads, int64_t grid, char *err,
                                       int32_t err_cap) {
  std::string e;
  SpiceyTimPlan p;
  bool ok = threads >= 1 && threads <= 1024 && (threads & (threads - 1)) == 0 && grid >= 0;
  if (!ok) e = "timing: bad arguments";
  ok = ok && spicey_tim_judge(n_inst, n_points, dt, v != nullptr, n_v, i != nullptr, n_i, reqs, n_req, out != nullptr,
                              work_bytes < 0 ? std::numeric_limits<int64_t>::max() : work_bytes, p, e);
  if (!ok) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  const int32_t n_edge = (int32_t)p.edges.size(), n_base = (int32_t)p.bases.size();
  auto blocks_of = [&](int64_t tiles) { return grid == 0 || grid > tiles ? tiles : grid; };
  // the base windows: the measurement pass, stats requests
  std::vector<double> base_out((size_t)n_inst * (size_t)(n_base ? n_base : 1) * 8, std::numeric_limits<double>::quiet_NaN());
  if (n_base > 0) {
    const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_base, threads);
    std::vector<double> partials((size_t)n_inst * (size_t)g.max_chunks * (size_t)n_base * 8, std::numeric_limits<double>::quiet_NaN());
    const int64_t blocks = blocks_of(g.tiles);
    for (int64_t b = 0; b < blocks; b++)
      for (int64_t tile = b; tile < g.tiles; tile += blocks)
        for (int32_t t = 0; t < threads; t++) spicey_meas_stage1(g, tile, t, p.bases.data(), n_base, n_points, dt, v, n_v, i, n_i, partials.data());
    for (int64_t idx = 0; idx < (int64_t)n_inst * n_base; idx++) spicey_meas_stage2(idx, p.bases.data(), n_base, g.max_chunks, partials.data(), base_out.data());
  }
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_edge, threads);
  std::vector<int32_t> counts((size_t)n_inst * (size_t)g.max_chunks * (size_t)n_edge, -1000000);
  const int64_t blocks = blocks_of(g.tiles);
  for (int64_t b = 0; b < blocks; b++)
    for (int64_t tile = b; tile < g.tiles; tile += blocks)
      for (int32_t t = 0; t < threads; t++)
        spicey_tim_stage1(g, tile, t, p.edges.data(), n_edge, n_base, n_points, v, n_v, i, n_i, base_out.data(), counts.data());
  for (int64_t idx = 0; idx < (int64_t)n_inst * n_req; idx++)
    spicey_tim_stage2(idx, p.reqs.data(), n_req, p.edges.data(), n_edge, n_base, g.max_chunks, n_points, dt, v, n_v, i, n_i, base_out.data(), counts.data(), out);
  return SPICEY_OK;
}
