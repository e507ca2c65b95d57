// values.h — the host side of the values pass: validation, the sorted tables and the workspace layout (values_exec.h holds
// the arithmetic and the mapping).  Plain C++, shared by spicey_abi.cpp, values.hip and the CPU harness of
// tests/values_host; the launcher of values.hip is declared at the end for translation units that have the HIP runtime's
// types.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "values_exec.h"

// Everything a launch needs, from the request list alone.
// workspace: point table | trace table | points table (the head, one upload) | trace partials [n_inst][total_items][6]
struct SpiceyValPlan {
  std::vector<SpiceyValDevTrace> traces;  // sorted by (signal, from, n, B, col)
  std::vector<SpiceyValDevPts> points;    // POINTS and FIND requests in the list's order
  int64_t n_pts = 0;                      // points of the table
  int64_t total_items = 0, max_items = 0, total_pitems = 0;
  int32_t max_B = 0, n_req = 0, longest_row = 0;
  int64_t off_traces = 0, off_points = 0, head_bytes = 0;
  int64_t workspace_bytes(int32_t n_inst) const {
    return head_bytes + spicey_meas_align((int64_t)n_inst * total_items * SPICEY_VAL_TRACE_DOUBLES * (int64_t)sizeof(double));
  }
};

// Checks every request and builds the tables; false + `err` for a list no launch accepts.  check_bufs = false leaves out
// what only the buffers decide (column ranges, the current buffer, the point table's values, the timing rows):
// spicey_values_workspace_bytes needs no more.
inline bool spicey_val_plan(const SpiceyValReq *reqs, int32_t n_req, int64_t n_points, const SpiceyValPoint *pts, int64_t n_pts, bool check_bufs, int32_t n_v,
                            int32_t n_i, bool have_i, bool have_timing, int32_t n_timing, SpiceyValPlan &p, std::string &err) {
  char buf[224];
  p = SpiceyValPlan();
  if (!reqs || n_req <= 0) { err = "values: n_req must be >= 1 and the request list not null"; return false; }
  if (n_points <= 0) { err = "values: n_points must be >= 1"; return false; }
  if (n_pts < 0 || (check_bufs && n_pts > 0 && !pts)) { err = "values: n_pts must be >= 0 and the point table not null when n_pts > 0"; return false; }
  if (check_bufs)
    for (int64_t j = 0; j < n_pts; j++) {
      const char *what = nullptr;
      if (pts[j].k < 0 || pts[j].k > n_points - 2) what = "k outside [0, n_points - 2]";
      else if (!(pts[j].f >= 0.0 && pts[j].f <= 1.0)) what = "f outside [0, 1] or not finite";
      if (what) {
        snprintf(buf, sizeof(buf), "values: point %lld: %s", (long long)j, what);
        err = buf;
        return false;
      }
    }
  int64_t longest = 0;
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyValReq &q = reqs[i];
    const char *what = nullptr;
    const int64_t to = q.step_to == -1 ? n_points - 1 : q.step_to;
    if (q.kind < 0 || q.kind > 2) what = "unknown kind (0 = trace, 1 = points, 2 = find)";
    else if (q.signal != 0 && q.signal != 1) what = "unknown signal (0 = out_v, 1 = out_i)";
    else if (q.kind == 2 && q.x_signal != 0 && q.x_signal != 1) what = "unknown signal of the edge (0 = out_v, 1 = out_i)";
    else if (q.reserved != 0) what = "reserved must be 0";
    else if (check_bufs && (q.signal == 1 || (q.kind == 2 && q.x_signal == 1)) && !have_i) what = "signal = 1 without a current buffer";
    else if (check_bufs) {
      const int32_t n = q.signal ? n_i : n_v, nx = q.x_signal ? n_i : n_v;
      if (q.col < 0 || q.col >= n || q.col_ref < -1 || q.col_ref >= n) what = "column out of range";
      else if (q.kind == 2 && (q.x_col < 0 || q.x_col >= nx || q.x_col_ref < -1 || q.x_col_ref >= nx)) what = "column of the edge out of range";
    }
    if (!what && q.kind == 0) {
      if (q.step_from < 0 || to < 0 || to >= n_points || q.step_from > to) what = "window outside [0, n_points) or step_from > step_to";
      else if (q.buckets < 1 || q.buckets > SPICEY_TRACE_MAX_BUCKETS || (int64_t)q.buckets > to - q.step_from + 1)
        what = "buckets outside 1 .. min(samples of the window, SPICEY_TRACE_MAX_BUCKETS)";
    } else if (!what && n_points < 2) {
      what = "points and find requests need n_points >= 2";
    } else if (!what && q.kind == 1) {
      if (q.first < 0 || q.count < 1 || q.first > n_pts || q.count > n_pts - q.first) what = "point run outside the table (count >= 1)";
      else if (q.count > (int64_t)(INT_MAX / SPICEY_VAL_POINT_DOUBLES)) what = "point run too long for a row";
    } else if (!what && check_bufs) {
      if (!have_timing) what = "a find request without timing rows";
      else if (q.timing_row < 0 || q.timing_row >= n_timing) what = "timing_row outside [0, n_timing)";
    }
    if (what) {
      snprintf(buf, sizeof(buf), "values: request %d: %s", (int)i, what);
      err = buf;
      p = SpiceyValPlan();
      return false;
    }
    if (q.kind == 0) {
      const int64_t n = to - q.step_from + 1;
      const int64_t longest_bucket = (n + q.buckets - 1) / q.buckets;
      p.traces.push_back(SpiceyValDevTrace{q.signal, q.col, q.col_ref, i, q.buckets, (int32_t)((longest_bucket + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK), q.step_from, n, 0});
      longest = std::max(longest, (int64_t)q.buckets * SPICEY_VAL_TRACE_DOUBLES);
    } else {
      const int64_t count = q.kind == 1 ? q.count : 1;
      p.points.push_back(SpiceyValDevPts{q.kind, q.signal, q.col, q.col_ref, q.x_signal, q.x_col, q.x_col_ref, q.timing_row, i, 0, q.kind == 1 ? q.first : 0, count,
                                         p.total_pitems});
      p.total_pitems += count;
      longest = std::max(longest, count * SPICEY_VAL_POINT_DOUBLES);
    }
  }
  // (neighbouring lanes read neighbouring columns of one row where the windows agree; a row does not depend on the order)
  std::stable_sort(p.traces.begin(), p.traces.end(), [](const SpiceyValDevTrace &x, const SpiceyValDevTrace &y) {
    if (x.signal != y.signal) return x.signal < y.signal;
    if (x.from != y.from) return x.from < y.from;
    if (x.n != y.n) return x.n < y.n;
    if (x.B != y.B) return x.B < y.B;
    return x.col < y.col;
  });
  for (SpiceyValDevTrace &t : p.traces) {
    t.pbase = p.total_items;
    p.total_items += spicey_val_items(t);
    p.max_items = std::max(p.max_items, spicey_val_items(t));
    p.max_B = std::max(p.max_B, t.B);
  }
  p.n_pts = n_pts;
  p.n_req = n_req;
  p.longest_row = (int32_t)longest;
  p.off_traces = spicey_meas_align(n_pts * (int64_t)sizeof(SpiceyValPoint));
  p.off_points = p.off_traces + spicey_meas_align((int64_t)p.traces.size() * (int64_t)sizeof(SpiceyValDevTrace));
  p.head_bytes = p.off_points + spicey_meas_align((int64_t)p.points.size() * (int64_t)sizeof(SpiceyValDevPts));
  return true;
}

// point table | tables | partials; -1 for arguments no launch accepts
inline int64_t spicey_val_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyValReq *reqs, int32_t n_req, int64_t n_pts) {
  SpiceyValPlan p;
  std::string err;
  if (n_inst <= 0 || !spicey_val_plan(reqs, n_req, n_points, nullptr, n_pts, false, 0, 0, false, false, 0, p, err)) return -1;
  return p.workspace_bytes(n_inst);
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing): counts, buffers, dt, the
// request list, the point table, the row length, the workspace size.  true: `p` holds the launch's tables.
inline bool spicey_val_judge(int32_t n_inst, int64_t n_points, double dt, bool have_v, int32_t n_v, bool have_i, int32_t n_i, const SpiceyValReq *reqs,
                             int32_t n_req, const SpiceyValPoint *pts, int64_t n_pts, bool have_timing, int32_t n_timing, bool have_out, int32_t out_stride,
                             int64_t work_bytes, SpiceyValPlan &p, std::string &err) {
  char buf[224];
  if (n_inst <= 0 || n_v < 0 || n_i < 0 || n_timing < 0 || !have_out) { err = "values: bad arguments (n_inst >= 1, result and workspace buffers)"; return false; }
  if (!(dt > 0.0) || !std::isfinite(dt)) { err = "values: dt must be finite and > 0"; return false; }
  if (!spicey_val_plan(reqs, n_req, n_points, pts, n_pts, true, have_v ? n_v : 0, n_i, have_i, have_timing, n_timing, p, err)) return false;
  if (out_stride < p.longest_row) {
    snprintf(buf, sizeof(buf), "values: out_stride %d is shorter than the longest request's %d doubles", (int)out_stride, (int)p.longest_row);
    err = buf;
    return false;
  }
  const int64_t need = p.workspace_bytes(n_inst);
  if (work_bytes < need) {
    snprintf(buf, sizeof(buf), "values: workspace of %lld bytes is too small, %lld needed (spicey_values_workspace_bytes)", (long long)work_bytes, (long long)need);
    err = buf;
    return false;
  }
  return true;
}

// The head of the workspace as one block of host memory: point table | trace table | points table.
inline void spicey_val_head(const SpiceyValPlan &p, const SpiceyValPoint *pts, std::vector<unsigned char> &head) {
  head.assign((size_t)p.head_bytes, 0);
  if (p.n_pts > 0) memcpy(head.data(), pts, (size_t)p.n_pts * sizeof(SpiceyValPoint));
  if (!p.traces.empty()) memcpy(head.data() + p.off_traces, p.traces.data(), p.traces.size() * sizeof(SpiceyValDevTrace));
  if (!p.points.empty()) memcpy(head.data() + p.off_points, p.points.data(), p.points.size() * sizeof(SpiceyValDevPts));
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The pass, enqueued on `st` behind a copy of the head (spicey_val_head of a plan spicey_val_judge accepted; pts: HOST)
// into d_work: the rows are cleared, then trace stage 1 and 2 (if the list has a trace) and the points kernel (if it has
// points or finds).  d_timing: DEVICE [n_inst][n_timing][8] or null.  The device must be current.  No synchronisation.
hipError_t spicey_launch_values(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                const SpiceyValPlan &plan, const SpiceyValPoint *pts, const double *d_timing, int32_t n_timing, double *d_out, int32_t out_stride,
                                void *d_work, hipStream_t st);
#endif
