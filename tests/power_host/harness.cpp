// CPU harness of the products of two signals: power_exec.h — the code the kernels of spicey_amd/csrc/power.hip run —
// through an emulation of their lane and chunk mapping: workgroups of `threads` threads take the stage 1 tiles blockIdx,
// blockIdx + grid, ..., every thread of a workgroup does what spicey_power_stage1 gives it, then one thread per (instance,
// request) combines (spicey_power_stage2).  The call is judged by spicey_power_judge of power.h, the judge of the library's
// entry points.  Compiled with -ffp-contract=off like the kernels' translation unit, so the results are the GPU's bit for
// bit.  The workspace starts as NaNs: a partial that is read without having been written shows.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/power.h"

extern "C" int32_t spicey_power_host_chunk(void) { return SPICEY_MEAS_CHUNK; }
extern "C" int32_t spicey_power_host_threads(void) { return SPICEY_MEAS_THREADS; }
extern "C" int64_t spicey_power_host_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  return spicey_pow_workspace_bytes(n_inst, n_points, n_req);
}

// threads: a power of two, 1 .. 1024; grid: workgroups launched, 0 = one per tile.  have_out = 0 stands for null result or
// workspace buffers, work_bytes = -1 for a workspace of exactly the size needed.  Returns SPICEY_OK or SPICEY_ERR_BAD_DESC
// (text in err; `rows` untouched).
extern "C" int32_t spicey_power_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                         const SpiceyPowerReq *reqs, int32_t n_req, double *rows, int32_t have_out, int64_t work_bytes, int32_t threads,
                                         int64_t grid, char *err, int32_t err_cap) {
  std::string e;
  std::vector<SpiceyPowerDevReq> table;
  bool ok = threads >= 1 && threads <= 1024 && (threads & (threads - 1)) == 0 && grid >= 0;
  if (!ok) e = "power: bad arguments of the emulated launch";
  const int64_t need = spicey_pow_workspace_bytes(n_inst, n_points, n_req);
  ok = ok && spicey_power_judge(n_inst, n_points, dt, v != nullptr, n_v, i != nullptr, n_i, reqs, n_req, have_out != 0 && rows, work_bytes < 0 ? need : work_bytes,
                                table, e);
  if (!ok) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  const int64_t head = spicey_power_head_bytes(n_req);
  std::vector<double> partials((size_t)(need - head) / sizeof(double), std::numeric_limits<double>::quiet_NaN());
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_req, threads);
  const int64_t blocks = grid == 0 || grid > g.tiles ? g.tiles : grid;
  for (int64_t b = 0; b < blocks; b++)
    for (int64_t tile = b; tile < g.tiles; tile += blocks)
      for (int32_t t = 0; t < threads; t++)
        spicey_power_stage1(g, tile, t, table.data(), n_req, n_points, v, n_v, i, n_i, partials.data());
  for (int64_t idx = 0; idx < (int64_t)n_inst * n_req; idx++) spicey_power_stage2(idx, table.data(), n_req, g.max_chunks, partials.data(), rows);
  return SPICEY_OK;
}
