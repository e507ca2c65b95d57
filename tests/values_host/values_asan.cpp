// The harness of the values pass behind a stand-alone program with its own main, for the address and undefined-behaviour
// sanitizers (`make asan`): the judge, the plan, the workspace layout, both trace stages and the points stage on heap
// buffers of exactly the stated sizes — samples, point table, timing rows, result rows (the harness sizes the head block
// and the partials exactly itself) — over shapes on either side of a sub-chunk, several emulated launches, and one refusal
// per kind of bad input.  CPU only; nothing of it is loaded into python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spicey_amd/csrc/values.h"

extern "C" int32_t spicey_values_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                          const SpiceyValReq *reqs, int32_t n_req, const SpiceyValPoint *pts, int64_t n_pts, const double *timing,
                                          int32_t n_timing, double *rows, int32_t out_stride, int32_t have_out, int64_t work_bytes, int32_t threads, int64_t grid,
                                          char *err, int32_t err_cap);

static SpiceyValReq req(int32_t kind, int32_t signal, int32_t col, int32_t col_ref) {
  SpiceyValReq q;
  memset(&q, 0, sizeof(q));
  q.kind = kind; q.signal = signal; q.col = col; q.col_ref = col_ref; q.x_col_ref = -1; q.step_to = -1; q.buckets = 1;
  return q;
}

int main() {
  const int32_t C = SPICEY_MEAS_CHUNK, n_inst = 3, n_v = 3, n_i = 2, n_timing = 2;
  const int64_t shapes[] = {2, 3, C - 1, C, C + 1, 3 * C + 7};
  const int32_t launches[][2] = {{256, 0}, {64, 0}, {1, 0}, {1024, 0}, {256, 1}, {128, 3}};
  char err[256];
  int runs = 0, refusals = 0;
  for (const int64_t np : shapes) {
    std::vector<double> v((size_t)n_inst * np * n_v), ci((size_t)n_inst * np * n_i), timing((size_t)n_inst * n_timing * 8, -1.0);
    for (size_t k = 0; k < v.size(); k++) v[k] = std::sin(0.37 * (double)k);
    for (size_t k = 0; k < ci.size(); k++) ci[k] = std::cos(0.11 * (double)k);
    for (int32_t in = 0; in < n_inst; in++) {  // row 0: a crossing in the run's last interval; row 1: none; instance 2: a k beyond the run
      double *row = timing.data() + (size_t)in * n_timing * 8;
      row[3] = in == 2 ? (double)np : (double)(np - 2);
      row[5] = 0.25;
    }
    std::vector<SpiceyValPoint> pts = {{0, 0.0}, {0, 1.0}, {np - 2, 0.5}, {np - 2, 1.0}, {(np - 2) / 2, 0.75}};
    std::vector<SpiceyValReq> reqs;
    const int64_t Bs[] = {1, 2, 3, 7, 64, 65, np};
    for (const int64_t B : Bs) {
      SpiceyValReq q = req(SPICEY_VAL_TRACE, (int32_t)(B & 1), 1, B % 3 == 0 ? 0 : -1);
      q.buckets = (int32_t)(B < np ? B : np);
      reqs.push_back(q);
      if (np > 5) {  // a window that starts and ends inside the run
        q.step_from = 2; q.step_to = np - 3;
        q.buckets = (int32_t)(B < np - 4 ? B : np - 4);
        reqs.push_back(q);
      }
    }
    SpiceyValReq p = req(SPICEY_VAL_POINTS, 0, 2, 0);
    p.first = 0; p.count = (int64_t)pts.size();
    reqs.push_back(p);
    p.signal = 1; p.col = 1; p.col_ref = -1; p.first = 4; p.count = 1;
    reqs.push_back(p);
    for (int32_t t = 0; t < n_timing; t++) {
      SpiceyValReq f = req(SPICEY_VAL_FIND, 1, 0, 1);
      f.x_signal = 0; f.x_col = 2; f.x_col_ref = t ? 0 : -1; f.timing_row = t;
      reqs.push_back(f);
    }
    int64_t stride = 4 * (int64_t)pts.size();
    for (const SpiceyValReq &q : reqs)
      if (q.kind == SPICEY_VAL_TRACE && 6 * (int64_t)q.buckets > stride) stride = 6 * (int64_t)q.buckets;
    for (const auto &l : launches) {
      std::vector<double> rows((size_t)n_inst * reqs.size() * (size_t)stride);
      const int32_t rc = spicey_values_host_run(n_inst, np, 1e-6, v.data(), n_v, ci.data(), n_i, reqs.data(), (int32_t)reqs.size(), pts.data(), (int64_t)pts.size(),
                                                timing.data(), n_timing, rows.data(), (int32_t)stride, 1, -1, l[0], l[1], err, sizeof(err));
      if (rc != SPICEY_OK) { fprintf(stderr, "n_points %lld: unexpected refusal: %s\n", (long long)np, err); return 1; }
      // the find rows: found in the last interval for instances 0 and 1 of row 0, not found elsewhere
      for (int32_t in = 0; in < n_inst; in++)
        for (int32_t t = 0; t < n_timing; t++) {
          const double k = rows[((size_t)in * reqs.size() + reqs.size() - 2 + t) * (size_t)stride];
          if (k != (t == 0 && in != 2 ? (double)(np - 2) : -1.0)) { fprintf(stderr, "n_points %lld: find row (%d, %d) has k = %g\n", (long long)np, in, t, k); return 1; }
        }
      runs++;
    }
    // refusals leave before anything is touched: a bucket count above the window, a point beyond the run, a short row
    std::vector<double> rows((size_t)n_inst * reqs.size() * (size_t)stride);
    std::vector<SpiceyValReq> bad = reqs;
    bad[0].buckets = (int32_t)np + 1;
    refusals += spicey_values_host_run(n_inst, np, 1e-6, v.data(), n_v, ci.data(), n_i, bad.data(), (int32_t)bad.size(), pts.data(), (int64_t)pts.size(), timing.data(),
                                       n_timing, rows.data(), (int32_t)stride, 1, -1, 256, 0, err, sizeof(err)) == SPICEY_ERR_BAD_DESC;
    std::vector<SpiceyValPoint> far = pts;
    far[2].k = np - 1;
    refusals += spicey_values_host_run(n_inst, np, 1e-6, v.data(), n_v, ci.data(), n_i, reqs.data(), (int32_t)reqs.size(), far.data(), (int64_t)far.size(), timing.data(),
                                       n_timing, rows.data(), (int32_t)stride, 1, -1, 256, 0, err, sizeof(err)) == SPICEY_ERR_BAD_DESC;
    refusals += spicey_values_host_run(n_inst, np, 1e-6, v.data(), n_v, ci.data(), n_i, reqs.data(), (int32_t)reqs.size(), pts.data(), (int64_t)pts.size(), timing.data(),
                                       n_timing, rows.data(), (int32_t)stride - 1, 1, -1, 256, 0, err, sizeof(err)) == SPICEY_ERR_BAD_DESC;
  }
  if (refusals != 3 * (int)(sizeof(shapes) / sizeof(shapes[0]))) { fprintf(stderr, "%d refusals\n", refusals); return 1; }
  printf("values_asan: %d runs and %d refusals clean\n", runs, refusals);
  return 0;
}
