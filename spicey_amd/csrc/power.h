// power.h — the host side of the product pass: validation, the sorted table and the workspace layout (power_exec.h holds
// the arithmetic and the mapping).  Plain C++, shared by spicey_abi.cpp, power.hip and the CPU harness of tests/power_host;
// the launcher of power.hip is declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "power_exec.h"

// bytes of the request table at the head of the workspace
inline int64_t spicey_power_head_bytes(int32_t n_req) { return spicey_meas_align((int64_t)n_req * (int64_t)sizeof(SpiceyPowerDevReq)); }

// table | partials [n_inst][max_chunks][n_req][16]; -1 for arguments no launch accepts
inline int64_t spicey_pow_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  if (n_inst <= 0 || n_points <= 0 || n_req <= 0) return -1;
  const int64_t max_chunks = (n_points + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK;
  return spicey_power_head_bytes(n_req) + spicey_meas_align((int64_t)n_inst * max_chunks * (int64_t)n_req * SPICEY_POWER_ROW * (int64_t)sizeof(double));
}

// Checks every request and builds the kernels' table; false + `err` for a request no launch accepts.  n_v = 0 where there
// is no voltage buffer.
inline bool spicey_power_plan(const SpiceyPowerReq *reqs, int32_t n_req, int64_t n_points, int32_t n_v, int32_t n_i, bool have_i,
                              std::vector<SpiceyPowerDevReq> &table, std::string &err) {
  char buf[200];
  table.clear();
  if (!reqs || n_req <= 0) { err = "power: n_req must be >= 1 and the request list not null"; return false; }
  if (n_points <= 0) { err = "power: n_points must be >= 1"; return false; }
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyPowerReq &q = reqs[i];
    const char *what = nullptr;
    if ((q.a_signal != 0 && q.a_signal != 1) || (q.b_signal != 0 && q.b_signal != 1)) what = "unknown signal (0 = out_v, 1 = out_i)";
    else if ((q.a_signal == 1 || q.b_signal == 1) && !have_i) what = "signal = 1 without a current buffer";
    else if (q.neg != 0 && q.neg != 1) what = "neg must be 0 or 1";
    else if (q.reserved != 0) what = "reserved must be 0";
    const int64_t to = q.step_to == -1 ? n_points - 1 : q.step_to;
    if (!what) {
      const int32_t na = q.a_signal ? n_i : n_v, nb = q.b_signal ? n_i : n_v;
      if (q.a_col < 0 || q.a_col >= na || q.a_col_ref < -1 || q.a_col_ref >= na || q.b_col < 0 || q.b_col >= nb || q.b_col_ref < -1 || q.b_col_ref >= nb)
        what = "column out of range";
      else if (q.step_from < 0 || to < 0 || to >= n_points || q.step_from > to) what = "window outside [0, n_points) or step_from > step_to";
    }
    if (what) {
      snprintf(buf, sizeof(buf), "power: request %d: %s", (int)i, what);
      err = buf;
      table.clear();
      return false;
    }
    table.push_back(SpiceyPowerDevReq{q.a_signal, q.a_col, q.a_col_ref, q.b_signal, q.b_col, q.b_col_ref, q.neg, i, q.step_from, to});
  }
  // (neighbouring lanes read neighbouring columns of one row; a row of the result does not depend on the order)
  std::stable_sort(table.begin(), table.end(), [](const SpiceyPowerDevReq &x, const SpiceyPowerDevReq &y) {
    if (x.a_signal != y.a_signal) return x.a_signal < y.a_signal;
    if (x.a_col != y.a_col) return x.a_col < y.a_col;
    if (x.b_signal != y.b_signal) return x.b_signal < y.b_signal;
    return x.b_col < y.b_col;
  });
  return true;
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing): counts, buffers, dt, the
// request list, the workspace size.  true: `table` is the kernels'.
inline bool spicey_power_judge(int32_t n_inst, int64_t n_points, double dt, bool have_v, int32_t n_v, bool have_i, int32_t n_i, const SpiceyPowerReq *reqs,
                               int32_t n_req, bool have_out, int64_t work_bytes, std::vector<SpiceyPowerDevReq> &table, std::string &err) {
  table.clear();
  if (n_inst <= 0 || n_v < 0 || n_i < 0 || !have_out) { err = "power: bad arguments (n_inst >= 1, result and workspace buffers)"; return false; }
  if (!(dt > 0.0) || !std::isfinite(dt)) { err = "power: dt must be finite and > 0"; return false; }
  if (!spicey_power_plan(reqs, n_req, n_points, have_v ? n_v : 0, n_i, have_i, table, err)) return false;
  const int64_t need = spicey_pow_workspace_bytes(n_inst, n_points, n_req);
  if (work_bytes < need) {
    char buf[192];
    snprintf(buf, sizeof(buf), "power: workspace of %lld bytes is too small, %lld needed (spicey_power_workspace_bytes)", (long long)work_bytes, (long long)need);
    err = buf;
    table.clear();
    return false;
  }
  return true;
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The two kernels of the product pass, enqueued on `st` behind a copy of `table` (HOST, validated and sorted:
// spicey_power_judge) into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_power(int device, int32_t n_inst, int64_t n_points, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                               const SpiceyPowerDevReq *table, int32_t n_req, double *d_out, void *d_work, hipStream_t st);
#endif
