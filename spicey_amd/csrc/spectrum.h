// spectrum.h — the host side of the spectrum pass: the twiddle and window tables, validation, the launch plan and the
// workspace layout (spectrum_exec.h holds the arithmetic).  Plain C++, shared by spicey_abi.cpp, spectrum.hip and the CPU
// harness of tests/spectrum_host; the launcher of spectrum.hip is declared at the end for translation units that have
// the HIP runtime's types.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "spectrum_exec.h"

// T[k] = (cos((2.0 M_PI k) / N), -sin((2.0 M_PI k) / N)), k < N/2, interleaved {re, im}; T[0] and T[N/4] exact.
// (cos and sin proper, kept apart through a volatile copy: see spicey_four_twiddle of fourier_exec.h.)
inline void spicey_spec_twiddles(int32_t log2n, double *T) {
  const int32_t N = 1 << log2n;
  for (int32_t k = 0; k < N / 2; k++) {
    const double a = ((2.0 * M_PI) * (double)k) / (double)N;
    volatile double a_again = a;
    T[2 * k] = std::cos(a);
    T[2 * k + 1] = -std::sin(a_again);
  }
  T[0] = 1.0;
  T[1] = 0.0;
  T[2 * (N / 4)] = 0.0;
  T[2 * (N / 4) + 1] = -1.0;
}

// The periodic Hann window w_j = 0.5 - 0.5 cos((2.0 M_PI j) / N), j < N.
inline void spicey_spec_hann(int32_t log2n, double *w) {
  const int32_t N = 1 << log2n;
  for (int32_t j = 0; j < N; j++) {
    const double c = 0.5 * std::cos(((2.0 * M_PI) * (double)j) / (double)N);
    w[j] = 0.5 - c;
  }
}

// Everything a launch needs, from the request list alone.  One kernel launch per distinct N (its dynamic LDS is 16 N bytes):
// `order` lists the requests grouped by ascending log2n, in the caller's order inside a group, and launch L takes
// order[first .. first + count).  Head of the workspace: table | order | tables, each aligned; nothing behind it.
struct SpiceySpecLaunch {
  int32_t log2n, first, count;
};
struct SpiceySpecPlan {
  std::vector<SpiceySpecDevReq> table;  // the caller's order
  std::vector<int32_t> order;
  std::vector<SpiceySpecLaunch> launches;
  int32_t tw_off[SPICEY_SPEC_MAX_LOG2N + 1], win_off[SPICEY_SPEC_MAX_LOG2N + 1];  // per log2n, doubles into the table area; -1: not needed
  int32_t max_row = 0;
  int64_t table_doubles = 0;
  int64_t off_order = 0, off_tables = 0, head_bytes = 0;
  int64_t workspace_bytes() const { return head_bytes; }
};

// What the request list alone decides — lengths, windows, kinds, bands, first steps — checked, and the layout built from
// it (spicey_spectrum_workspace_bytes needs no more).  false + `err` for a list no launch accepts.
inline bool spicey_spec_layout(const SpiceySpecReq *reqs, int32_t n_req, int64_t n_points, SpiceySpecPlan &p, std::string &err) {
  char buf[200];
  p = SpiceySpecPlan();
  for (int32_t l = 0; l <= SPICEY_SPEC_MAX_LOG2N; l++) p.tw_off[l] = p.win_off[l] = -1;
  if (!reqs || n_req <= 0) { err = "spectrum: n_req must be >= 1 and the request list not null"; return false; }
  if (n_points <= 0) { err = "spectrum: n_points must be >= 1"; return false; }
  bool need_tw[SPICEY_SPEC_MAX_LOG2N + 1] = {}, need_win[SPICEY_SPEC_MAX_LOG2N + 1] = {};
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceySpecReq &q = reqs[i];
    const char *what = nullptr;
    if (q.log2n < SPICEY_SPEC_MIN_LOG2N || q.log2n > SPICEY_SPEC_MAX_LOG2N) what = "log2n outside 3..13";
    else if (q.kind != 0 && q.kind != 1) what = "unknown kind (0 = bins, 1 = dominant)";
    else if (q.window != 0 && q.window != 1) what = "unknown window (0 = rectangular, 1 = Hann)";
    else if (q.step_from < 0 || q.step_from > n_points - ((int64_t)1 << q.log2n)) what = "step_from < 0 or step_from + N > n_points";
    else if (q.bin_from < 0 || q.bin_to > (1 << q.log2n) / 2 || q.bin_from > q.bin_to) what = "band outside [0, N/2] or bin_from > bin_to";
    if (what) {
      snprintf(buf, sizeof(buf), "spectrum: request %d: %s", (int)i, what);
      err = buf;
      return false;
    }
    need_tw[q.log2n] = true;
    if (q.window == 1) need_win[q.log2n] = true;
    p.max_row = std::max(p.max_row, spicey_spec_row_doubles(q.kind, q.bin_from, q.bin_to));
  }
  for (int32_t l = SPICEY_SPEC_MIN_LOG2N; l <= SPICEY_SPEC_MAX_LOG2N; l++) {
    if (!need_tw[l]) continue;
    p.tw_off[l] = (int32_t)p.table_doubles;
    p.table_doubles += (int64_t)1 << l;  // N/2 pairs
    if (need_win[l]) {
      p.win_off[l] = (int32_t)p.table_doubles;
      p.table_doubles += (int64_t)1 << l;
    }
    SpiceySpecLaunch L{l, (int32_t)p.order.size(), 0};
    for (int32_t i = 0; i < n_req; i++)
      if (reqs[i].log2n == l) p.order.push_back(i);
    L.count = (int32_t)p.order.size() - L.first;
    p.launches.push_back(L);
  }
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceySpecReq &q = reqs[i];
    p.table.push_back(SpiceySpecDevReq{q.signal, q.col, q.col_ref, q.kind, q.step_from, q.log2n, q.window, q.bin_from, q.bin_to, p.tw_off[q.log2n],
                                       q.window == 1 ? p.win_off[q.log2n] : -1});
  }
  p.off_order = spicey_meas_align((int64_t)n_req * (int64_t)sizeof(SpiceySpecDevReq));
  p.off_tables = p.off_order + spicey_meas_align((int64_t)n_req * (int64_t)sizeof(int32_t));
  p.head_bytes = p.off_tables + spicey_meas_align(p.table_doubles * (int64_t)sizeof(double));
  return true;
}

// table | order | tables; -1 for arguments no launch accepts
inline int64_t spicey_spec_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceySpecReq *reqs, int32_t n_req) {
  SpiceySpecPlan p;
  std::string err;
  if (n_inst <= 0 || !spicey_spec_layout(reqs, n_req, n_points, p, err)) return -1;
  return p.workspace_bytes();
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing): counts, buffers, the request
// list, dt, the row stride, the workspace size.  true: `p` holds the launch's tables.
inline bool spicey_spec_judge(int32_t n_inst, int64_t n_points, double dt, bool have_v, int32_t n_v, bool have_i, int32_t n_i, const SpiceySpecReq *reqs,
                              int32_t n_req, bool have_out, int32_t out_stride, int64_t work_bytes, SpiceySpecPlan &p, std::string &err) {
  char buf[224];
  if (n_inst <= 0 || n_v < 0 || n_i < 0 || !have_out) { err = "spectrum: bad arguments (n_inst >= 1, result and workspace buffers)"; return false; }
  if (!(dt > 0.0) || !std::isfinite(dt)) { err = "spectrum: dt must be finite and > 0"; return false; }
  if (!spicey_spec_layout(reqs, n_req, n_points, p, err)) return false;
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceySpecReq &q = reqs[i];
    const char *what = nullptr;
    if (q.signal != 0 && q.signal != 1) what = "unknown signal (0 = out_v, 1 = out_i)";
    else if (q.signal == 1 && !have_i) what = "signal = 1 without a current buffer";
    else {
      const int32_t n = q.signal ? n_i : (have_v ? n_v : 0);
      if (q.col < 0 || q.col >= n || q.col_ref < -1 || q.col_ref >= n) what = "column out of range";
    }
    if (what) {
      snprintf(buf, sizeof(buf), "spectrum: request %d: %s", (int)i, what);
      err = buf;
      return false;
    }
  }
  if (out_stride < p.max_row) {
    snprintf(buf, sizeof(buf), "spectrum: out_stride %d is too small, %d needed (2 bins of the widest band, 8 for a dominant)", (int)out_stride, (int)p.max_row);
    err = buf;
    return false;
  }
  const int64_t need = p.workspace_bytes();
  if (work_bytes < need) {
    snprintf(buf, sizeof(buf), "spectrum: workspace of %lld bytes is too small, %lld needed (spicey_spectrum_workspace_bytes)", (long long)work_bytes, (long long)need);
    err = buf;
    return false;
  }
  return true;
}

// The head of the workspace as one block of host memory: table | order | tables (built here, by the host's libm).
inline void spicey_spec_head(const SpiceySpecPlan &p, std::vector<unsigned char> &head) {
  head.assign((size_t)p.head_bytes, 0);
  memcpy(head.data(), p.table.data(), p.table.size() * sizeof(SpiceySpecDevReq));
  memcpy(head.data() + p.off_order, p.order.data(), p.order.size() * sizeof(int32_t));
  double *tables = (double *)(head.data() + p.off_tables);
  for (int32_t l = SPICEY_SPEC_MIN_LOG2N; l <= SPICEY_SPEC_MAX_LOG2N; l++) {
    if (p.tw_off[l] >= 0) spicey_spec_twiddles(l, tables + p.tw_off[l]);
    if (p.win_off[l] >= 0) spicey_spec_hann(l, tables + p.win_off[l]);
  }
}

// Dynamic LDS of a launch for N = 2^log2n: the two planes.
inline size_t spicey_spec_lds_bytes(int32_t log2n) { return (size_t)16 << log2n; }

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The launches of the spectrum pass (one per distinct N of the plan), enqueued on `st` behind a copy of the plan's head
// (HOST: spicey_spec_judge) into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_spectrum(int device, int32_t n_inst, int64_t n_points, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                  const SpiceySpecPlan &plan, double *d_out, int32_t out_stride, void *d_work, hipStream_t st);
#endif
