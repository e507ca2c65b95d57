// ac_measure_exec.h — measurements over the complex outputs of an AC sweep: the one definition of the reduction, used by
// the kernel of ac_measure.hip and by the CPU harness of tests/ac_measure_host (compiled without FMA contraction on both
// sides, so the two give the same bits).
//
// A request (SpiceyAcMeasReq, include/spicey_hip.h) names one complex signal H_k = num_k or num_k / den_k over the frequency
// indices k of out_v / out_i [n_inst][n_freq][n][2], the real quantity q_k measured on it (|H|^2, re or im) and an
// inclusive window [from, to].  Per (instance, request) 8 doubles come out:
//   extrema    {min, max, k_min, k_max, re@k_min, im@k_min, re@k_max, im@k_max} — what m = q_from followed by the plain
//              comparisons q < m, q > m in ascending k gives: the first occurrence wins, a NaN sample never replaces an
//              extreme, a NaN first sample stays;
//   crossings  {count, k_first, k_last, re_k, im_k, re_k+1, im_k+1, thr} over the intervals (k, k + 1) inside the window.
//
// Mapping.  The reduction axis is short (tens to a few thousand frequencies) and the parallel axis long (instances x
// requests), so one WAVE takes one (instance, request) pair: lane l walks k = from + l, from + l + lanes, ... in ascending
// order and keeps a partial (spicey_acm_lane); the partials meet in a butterfly of cross-lane moves (spicey_acm_combine);
// lane 0 re-reads the samples its result names and writes the row (spicey_acm_finish).  Nothing is accumulated in floating
// point and spicey_acm_combine is commutative and associative — smaller value, or equal value and lower k; integer count,
// min / max of indices — so a row is a function of the window's samples and the request alone, whatever the lane count, the
// grid, n_inst or the other requests are.  No atomics, no workgroup ever waits for another, no partials in memory.
#pragma once
#include <stdint.h>

#include "../../include/spicey_hip.h"

#if defined(__HIPCC__)
#define SPICEY_ACM_HD __host__ __device__ __forceinline__
#else
#define SPICEY_ACM_HD inline
#endif

#define SPICEY_ACM_LANES 64     // lanes that share one (instance, request) pair: a wave
#define SPICEY_ACM_THREADS 256  // workgroup size: 4 pairs per workgroup
#define SPICEY_ACM_HEAD_ALIGN 256
#define SPICEY_ACM_NONE INT64_MAX  // "no sample yet" / "no crossing yet" in a partial's k0

// A validated request as the kernel reads it: the table is sorted by (num_signal, num_col), `orig` is the request's place
// in the caller's list (the row of `meas` it fills), `to` is resolved.
struct SpiceyAcMeasDevReq {
  int32_t kind, what, num_signal, num_col, num_col_ref, den_signal, den_col, den_col_ref;
  int32_t dir, which, rel, orig;
  int64_t from, to;
  double level;
};

// the sweep's buffers: a_v [n_inst][n_freq][n_v][2], a_i [n_inst][n_freq][n_i][2] (or null)
struct SpiceyAcmBufs {
  const double *a_v, *a_i;
  int32_t n_v, n_i;
  int64_t n_freq;
};

struct SpiceyAcmCx { double re, im; };

// a lane's (and, combined, a pair's) partial.  extrema: v0 / k0 = smallest sample so far and its first k, v1 / k1 the
// largest (k0 = k1 = SPICEY_ACM_NONE: no non-NaN sample seen); crossings: cnt, k0 = first hit (NONE: none), k1 = last (-1)
struct SpiceyAcmPart {
  double v0, v1;
  int64_t k0, k1, cnt;
};

SPICEY_ACM_HD SpiceyAcmCx spicey_acm_term(const SpiceyAcmBufs &B, int32_t signal, int32_t col, int32_t col_ref, int64_t inst, int64_t k) {
  const int64_t n = signal ? B.n_i : B.n_v;
  const double *row = (signal ? B.a_i : B.a_v) + (inst * B.n_freq + k) * n * 2;
  SpiceyAcmCx z{row[2 * (int64_t)col], row[2 * (int64_t)col + 1]};
  if (col_ref >= 0) {
    z.re = z.re - row[2 * (int64_t)col_ref];
    z.im = z.im - row[2 * (int64_t)col_ref + 1];
  }
  return z;
}

// H_k of the request (Complex.div of math/Complex.ts:38-47 without its throw)
SPICEY_ACM_HD SpiceyAcmCx spicey_acm_h(const SpiceyAcmBufs &B, const SpiceyAcMeasDevReq &q, int64_t inst, int64_t k) {
  const SpiceyAcmCx a = spicey_acm_term(B, q.num_signal, q.num_col, q.num_col_ref, inst, k);
  if (q.den_signal < 0) return a;
  const SpiceyAcmCx b = spicey_acm_term(B, q.den_signal, q.den_col, q.den_col_ref, inst, k);
  const double d = b.re * b.re + b.im * b.im;
  return SpiceyAcmCx{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}

SPICEY_ACM_HD double spicey_acm_q(const SpiceyAcmCx &h, int32_t what) { return what == 0 ? h.re * h.re + h.im * h.im : what == 1 ? h.re : h.im; }

SPICEY_ACM_HD double spicey_acm_qk(const SpiceyAcmBufs &B, const SpiceyAcMeasDevReq &q, int64_t inst, int64_t k) {
  return spicey_acm_q(spicey_acm_h(B, q, inst, k), q.what);
}

// the threshold of a crossings request (0 for extrema)
SPICEY_ACM_HD double spicey_acm_thr(const SpiceyAcmBufs &B, const SpiceyAcMeasDevReq &q, int64_t inst) {
  if (q.kind == 0) return 0.0;
  return q.rel ? q.level * spicey_acm_qk(B, q, inst, q.from) : q.level;
}

// What lane `lane` of `lanes` sees of the window, k ascending.
SPICEY_ACM_HD SpiceyAcmPart spicey_acm_lane(const SpiceyAcmBufs &B, const SpiceyAcMeasDevReq &q, int64_t inst, int32_t lane, int32_t lanes, double thr) {
  SpiceyAcmPart p{0.0, 0.0, SPICEY_ACM_NONE, SPICEY_ACM_NONE, 0};
  if (q.kind == 0) {
    for (int64_t k = q.from + lane; k <= q.to; k += lanes) {
      const double x = spicey_acm_qk(B, q, inst, k);
      if (x != x) continue;  // (q < m and q > m are both false for a NaN)
      if (p.k0 == SPICEY_ACM_NONE) { p.v0 = x; p.v1 = x; p.k0 = k; p.k1 = k; continue; }
      if (x < p.v0) { p.v0 = x; p.k0 = k; }
      if (x > p.v1) { p.v1 = x; p.k1 = k; }
    }
  } else {
    p.k1 = -1;
    const bool rise = q.dir >= 0, fall = q.dir <= 0;
    for (int64_t k = q.from + lane; k < q.to; k += lanes) {
      const double a = spicey_acm_qk(B, q, inst, k), b = spicey_acm_qk(B, q, inst, k + 1);
      if ((rise && a < thr && b >= thr) || (fall && a > thr && b <= thr)) {
        if (p.k0 == SPICEY_ACM_NONE) p.k0 = k;
        p.k1 = k;
        p.cnt = p.cnt + 1;
      }
    }
  }
  return p;
}

// p <- p combined with o: commutative and associative, so the order in which partials meet does not matter.
SPICEY_ACM_HD void spicey_acm_combine(int32_t kind, SpiceyAcmPart &p, const SpiceyAcmPart &o) {
  if (kind == 0) {
    if (o.k0 == SPICEY_ACM_NONE) return;
    if (p.k0 == SPICEY_ACM_NONE) { p = o; return; }
    if (o.v0 < p.v0 || (o.v0 == p.v0 && o.k0 < p.k0)) { p.v0 = o.v0; p.k0 = o.k0; }
    if (o.v1 > p.v1 || (o.v1 == p.v1 && o.k1 < p.k1)) { p.v1 = o.v1; p.k1 = o.k1; }
  } else {
    p.cnt = p.cnt + o.cnt;
    if (o.k0 < p.k0) p.k0 = o.k0;
    if (o.k1 > p.k1) p.k1 = o.k1;
  }
}

// The pair's row from its combined partial (one lane).
SPICEY_ACM_HD void spicey_acm_finish(const SpiceyAcmBufs &B, const SpiceyAcMeasDevReq &q, int64_t inst, const SpiceyAcmPart &p, double thr, double *out) {
  if (q.kind == 0) {
    const double x0 = spicey_acm_qk(B, q, inst, q.from);
    double mn = p.v0, mx = p.v1;
    int64_t kmn = p.k0, kmx = p.k1;
    if (x0 != x0) { mn = x0; mx = x0; kmn = q.from; kmx = q.from; }  // (m = q_from = NaN: no later comparison is true)
    const SpiceyAcmCx hn = spicey_acm_h(B, q, inst, kmn), hx = spicey_acm_h(B, q, inst, kmx);
    out[0] = mn; out[1] = mx; out[2] = (double)kmn; out[3] = (double)kmx;
    out[4] = hn.re; out[5] = hn.im; out[6] = hx.re; out[7] = hx.im;
  } else if (p.cnt == 0) {
    out[0] = 0.0; out[1] = -1.0; out[2] = -1.0;
    out[3] = 0.0; out[4] = 0.0; out[5] = 0.0; out[6] = 0.0; out[7] = thr;
  } else {
    const int64_t k = q.which ? p.k1 : p.k0;
    const SpiceyAcmCx ha = spicey_acm_h(B, q, inst, k), hb = spicey_acm_h(B, q, inst, k + 1);
    out[0] = (double)p.cnt; out[1] = (double)p.k0; out[2] = (double)p.k1;
    out[3] = ha.re; out[4] = ha.im; out[5] = hb.re; out[6] = hb.im; out[7] = thr;
  }
}

// ---- host side: validation, the sorted table, the workspace layout ---------------------------------------------------
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

// bytes of the request table, the whole workspace (the kernel keeps no partials); -1 for arguments no launch accepts
inline int64_t spicey_acm_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t n_req) {
  if (n_inst <= 0 || n_freq <= 0 || n_req <= 0) return -1;
  const int64_t b = (int64_t)n_req * (int64_t)sizeof(SpiceyAcMeasDevReq);
  return (b + SPICEY_ACM_HEAD_ALIGN - 1) / SPICEY_ACM_HEAD_ALIGN * SPICEY_ACM_HEAD_ALIGN;
}

// Checks every request and builds the kernel's table; false + `err` for a request no launch accepts.
inline bool spicey_acm_plan(const SpiceyAcMeasReq *reqs, int32_t n_req, int64_t n_freq, int32_t n_v, int32_t n_i, bool have_i,
                            std::vector<SpiceyAcMeasDevReq> &table, std::string &err) {
  char buf[200];
  table.clear();
  if (!reqs || n_req <= 0) { err = "ac measure: n_req must be >= 1 and the request list not null"; return false; }
  if (n_freq <= 0) { err = "ac measure: n_freq must be >= 1"; return false; }
  auto col_ok = [&](int32_t signal, int32_t col, int32_t col_ref) {
    const int32_t n = signal ? n_i : n_v;
    return col >= 0 && col < n && col_ref >= -1 && col_ref < n;
  };
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyAcMeasReq &q = reqs[i];
    const char *what = nullptr;
    const int64_t to = q.k_to == -1 ? n_freq - 1 : q.k_to;
    if (q.kind != 0 && q.kind != 1) what = "unknown kind (0 = extrema, 1 = crossings)";
    else if (q.num_signal != 0 && q.num_signal != 1) what = "unknown num_signal (0 = out_v, 1 = out_i)";
    else if (q.den_signal != -1 && q.den_signal != 0 && q.den_signal != 1) what = "unknown den_signal (-1 = none, 0 = out_v, 1 = out_i)";
    else if (q.what < 0 || q.what > 2) what = "unknown what (0 = |H|^2, 1 = re, 2 = im)";
    else if (q.dir != 0 && q.dir != 1 && q.dir != -1) what = "unknown dir (+1 rise, -1 fall, 0 either)";
    else if (q.which != 0 && q.which != 1) what = "unknown which (0 = first crossing, 1 = last)";
    else if (q.rel != 0 && q.rel != 1) what = "unknown rel (0 = absolute level, 1 = level times q at k_from)";
    else if (q.reserved != 0) what = "the reserved word must be 0";
    else if ((q.num_signal == 1 || q.den_signal == 1) && !have_i) what = "a current signal without a current buffer";
    else if (!col_ok(q.num_signal, q.num_col, q.num_col_ref) || (q.den_signal >= 0 && !col_ok(q.den_signal, q.den_col, q.den_col_ref)))
      what = "column out of range";
    else if (q.k_from < 0 || to < 0 || to >= n_freq || q.k_from > to) what = "window outside [0, n_freq) or k_from > k_to";
    if (what) {
      snprintf(buf, sizeof(buf), "ac measure: request %d: %s", (int)i, what);
      err = buf;
      table.clear();
      return false;
    }
    table.push_back(SpiceyAcMeasDevReq{q.kind, q.what, q.num_signal, q.num_col, q.num_col_ref, q.den_signal, q.den_col, q.den_col_ref, q.dir, q.which, q.rel,
                                       i, q.k_from, to, q.level});
  }
  // neighbouring waves read neighbouring columns of a row
  std::stable_sort(table.begin(), table.end(), [](const SpiceyAcMeasDevReq &a, const SpiceyAcMeasDevReq &b) {
    return a.num_signal != b.num_signal ? a.num_signal < b.num_signal : a.num_col < b.num_col;
  });
  return true;
}
