// values_exec.h — waveform VALUES over the step-major outputs of a transient run (a decimated trace, interpolated samples
// at given points, a second signal's value at a crossing the timing pass found): the one definition of the pass, used by
// the kernels of values.hip and by the CPU harness of tests/values_host (compiled without FMA contraction on both sides, so
// the two give the same bits).
//
// A request (SpiceyValReq, include/spicey_hip.h) names one signal y_k exactly as SpiceyMeasReq does and is of one of three
// kinds.
//   TRACE   the inclusive window [from, from + n - 1] cut into B buckets, bucket b = the steps from + floor(b n / B) ..
//           from + floor((b + 1) n / B) - 1 (64-bit products; B <= n, so no bucket is empty); per bucket {min, step_min,
//           max, step_max, first, last}.  The extremes follow the rule of measure_exec.h INSIDE a bucket: the bucket is cut
//           into sub-chunks of SPICEY_MEAS_CHUNK steps counted from ITS OWN first step, one thread walks a sub-chunk in
//           ascending step order from the sub-chunk's first sample with the plain comparisons x < m and x > m
//           (spicey_val_subchunk), the sub-chunk partials are combined in ascending order by the same comparisons
//           (spicey_val_bucket).  So the FIRST occurrence is named and a NaN behaves as under stats.
//   POINTS  a run of the shared point table {k, f}: d = y[k+1] - y[k]; value = y[k] for f == 0, y[k+1] for f == 1, else
//           y[k] + f d; slope = d / dt; every operation rounded on its own.  Per point {k, f, value, slope}.
//   FIND    the same at the crossing a timing row of THAT instance names: k = row[3], L = row[5], x the edge's own signal,
//           f = (L - x[k]) / (x[k+1] - x[k]) — the timing pass's own operations, so (k + f) dt is its t_targ.  A k outside
//           [0, n_points - 2] (the timing pass writes -1 for an edge it did not find) gives {-1, 0, 0, 0} and no sample is
//           read.
// No field is a floating-point accumulation: a row is a function of the samples, dt and the request alone (and, for FIND,
// of the instance's timing row) — not of n_inst, the thread count, the grid or the other requests of the list.
//
// Mapping.  A trace request owns items = B * S work items, S = ceil(ceil(n / B) / SPICEY_MEAS_CHUNK) sub-chunk slots per
// bucket (the longest bucket's need; a bucket one step shorter leaves at most one of them idle): item w is sub-chunk w % S
// of bucket w / S.  Stage 1 is the geometry of the measurement pass with items in the place of chunks: a workgroup is `rl`
// trace requests wide — the lanes of a wave first, and the table is sorted by (signal, from, n, B, col), so a wave
// instruction reads neighbouring columns of one row where the list allows — and `cl` items deep.  Every thread has its own
// loop bounds: a bucket that ends early ends that thread's loop and nobody else's.  Partials: [n_inst][all items][6], a
// request's items at `pbase`.  Stage 2: one thread per (instance, trace request, bucket).  Points kernel: one thread per
// (instance, item), the items of the POINTS and FIND requests (count, or 1) in one list; the request of an item by bisection
// of the `item0` column.
#pragma once
#include <stdint.h>

#include "measure_exec.h"

#define SPICEY_VAL_HD SPICEY_MEAS_HD
#define SPICEY_VAL_TRACE_DOUBLES 6  // per bucket, and per sub-chunk partial
#define SPICEY_VAL_POINT_DOUBLES 4  // per point

// A validated TRACE request as the kernels read it: `orig` is the request's place in the caller's list (the row of the
// result it fills), n the window's samples, S the sub-chunk slots of a bucket, pbase the first of its B * S partial slots.
struct SpiceyValDevTrace {
  int32_t signal, col, col_ref, orig;
  int32_t B, S;
  int64_t from, n, pbase;
};

// A validated POINTS (kind 1) or FIND (kind 2) request: first / count name the run of the point table (FIND: count = 1),
// item0 the first of its items in the points kernel's list.
struct SpiceyValDevPts {
  int32_t kind, signal, col, col_ref;
  int32_t x_signal, x_col, x_col_ref, timing_row;
  int32_t orig, pad;
  int64_t first, count, item0;
};

SPICEY_VAL_HD int64_t spicey_val_items(const SpiceyValDevTrace &q) { return (int64_t)q.B * q.S; }
SPICEY_VAL_HD int64_t spicey_val_bucket_lo(const SpiceyValDevTrace &q, int64_t b) { return q.from + b * q.n / q.B; }

// Stage 1 geometry: spicey_meas_geom with the longest request's items in the place of the run's chunks.
SPICEY_VAL_HD SpiceyMeasGeom spicey_val_geom(int32_t n_inst, int64_t max_items, int32_t n_trace, int32_t threads) {
  SpiceyMeasGeom g;
  g.rl = 1;
  while (g.rl < n_trace && g.rl < 64 && g.rl < threads) g.rl <<= 1;
  g.cl = threads / g.rl;
  g.max_chunks = max_items;
  g.r_tiles = ((int64_t)n_trace + g.rl - 1) / g.rl;
  g.c_tiles = (max_items + g.cl - 1) / g.cl;
  g.tiles = (int64_t)n_inst * g.r_tiles * g.c_tiles;
  return g;
}

// The steps lo .. hi (at most SPICEY_MEAS_CHUNK of them) in ascending order.  y(step) is the signal's sample (the
// subtraction included).  out: {min, step_min, max, step_max, first, last}.
template <class Load>
SPICEY_VAL_HD void spicey_val_subchunk(int64_t lo, int64_t hi, Load y, double *out) {
  const double y0 = y(lo);
  double mn = y0, mx = y0, last = y0;
  int64_t smn = lo, smx = lo;
  SPICEY_MEAS_UNROLL
  for (int64_t s = lo + 1; s <= hi; s++) {
    const double v = y(s);
    if (v < mn) { mn = v; smn = s; }
    if (v > mx) { mx = v; smx = s; }
    last = v;
  }
  out[0] = mn; out[1] = (double)smn; out[2] = mx; out[3] = (double)smx; out[4] = y0; out[5] = last;
}

// A bucket's `nsub` sub-chunk partials in ascending order.  p(sub) points at the 6 doubles of that sub-chunk.
template <class Get>
SPICEY_VAL_HD void spicey_val_bucket(int64_t nsub, Get p, double *out) {
  const double *p0 = p(0);
  double r[SPICEY_VAL_TRACE_DOUBLES];
  for (int j = 0; j < SPICEY_VAL_TRACE_DOUBLES; j++) r[j] = p0[j];
  for (int64_t c = 1; c < nsub; c++) {
    const double *pc = p(c);
    if (pc[0] < r[0]) { r[0] = pc[0]; r[1] = pc[1]; }
    if (pc[2] > r[2]) { r[2] = pc[2]; r[3] = pc[3]; }
    r[5] = pc[5];
  }
  for (int j = 0; j < SPICEY_VAL_TRACE_DOUBLES; j++) out[j] = r[j];
}

// What thread `t` of the workgroup working on `tile` does in trace stage 1 (nothing when it falls off the trace table, the
// request's items or its bucket's sub-chunks).  a_v / a_i: [n_inst][n_points][n_v | n_i]; total_items: the partial slots of
// one instance.
SPICEY_VAL_HD void spicey_val_stage1(const SpiceyMeasGeom &g, int64_t tile, int32_t t, const SpiceyValDevTrace *table, int32_t n_trace, int64_t total_items,
                                     int64_t n_points, const double *a_v, int32_t n_v, const double *a_i, int32_t n_i, double *partials) {
  const int64_t per_inst = g.r_tiles * g.c_tiles;
  const int64_t inst = tile / per_inst, rem = tile - inst * per_inst;
  const int64_t ct = rem / g.r_tiles, rt = rem - ct * g.r_tiles;
  const int64_t r = rt * g.rl + (t % g.rl), w = ct * g.cl + (t / g.rl);
  if (r >= n_trace) return;
  const SpiceyValDevTrace q = table[r];
  if (w >= spicey_val_items(q)) return;
  const int64_t b = w / q.S, sub = w - b * q.S;
  const int64_t lo = spicey_val_bucket_lo(q, b) + sub * SPICEY_MEAS_CHUNK, bhi = spicey_val_bucket_lo(q, b + 1) - 1;
  if (lo > bhi) return;  // (a slot the bucket does not need)
  const int64_t hi = lo + SPICEY_MEAS_CHUNK - 1 < bhi ? lo + SPICEY_MEAS_CHUNK - 1 : bhi;
  const int64_t n = q.signal ? n_i : n_v;
  const double *base = (q.signal ? a_i : a_v) + inst * n_points * n;
  double out[SPICEY_VAL_TRACE_DOUBLES];
  if (q.col_ref < 0) {
    const double *pa = base + q.col;
    spicey_val_subchunk(lo, hi, [=](int64_t s) { return pa[s * n]; }, out);
  } else {
    const double *pa = base + q.col, *pb = base + q.col_ref;
    spicey_val_subchunk(lo, hi, [=](int64_t s) { return pa[s * n] - pb[s * n]; }, out);
  }
  double *dst = partials + (inst * total_items + q.pbase + w) * SPICEY_VAL_TRACE_DOUBLES;
  for (int j = 0; j < SPICEY_VAL_TRACE_DOUBLES; j++) dst[j] = out[j];
}

// Trace stage 2, one thread per (instance, trace request, bucket): idx = (inst * n_trace + r) * max_B + b (nothing for
// b >= the request's B).
SPICEY_VAL_HD void spicey_val_stage2(int64_t idx, const SpiceyValDevTrace *table, int32_t n_trace, int32_t max_B, int64_t total_items, int32_t n_req,
                                     const double *partials, double *rows, int32_t out_stride) {
  const int64_t ir = idx / max_B, b = idx - ir * max_B;
  const int64_t inst = ir / n_trace, r = ir - inst * n_trace;
  const SpiceyValDevTrace q = table[r];
  if (b >= q.B) return;
  const int64_t len = spicey_val_bucket_lo(q, b + 1) - spicey_val_bucket_lo(q, b);
  const double *src = partials + (inst * total_items + q.pbase + b * q.S) * SPICEY_VAL_TRACE_DOUBLES;
  double out[SPICEY_VAL_TRACE_DOUBLES];
  spicey_val_bucket((len + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK, [=](int64_t c) { return src + c * SPICEY_VAL_TRACE_DOUBLES; }, out);
  double *dst = rows + (inst * n_req + q.orig) * (int64_t)out_stride + b * SPICEY_VAL_TRACE_DOUBLES;
  for (int j = 0; j < SPICEY_VAL_TRACE_DOUBLES; j++) dst[j] = out[j];
}

// value and slope of y at k + f.  out: {k, f, value, slope}.
template <class Load>
SPICEY_VAL_HD void spicey_val_point(int64_t k, double f, double dt, Load y, double *out) {
  const double y0 = y(k), y1 = y(k + 1);
  const double d = y1 - y0;
  const double part = f * d;
  out[0] = (double)k;
  out[1] = f;
  out[2] = f == 0.0 ? y0 : f == 1.0 ? y1 : y0 + part;
  out[3] = d / dt;
}

// The request that holds item `it` of the points kernel's list: the last one whose item0 <= it.
SPICEY_VAL_HD int32_t spicey_val_find_req(const SpiceyValDevPts *table, int32_t n_preq, int64_t it) {
  int32_t lo = 0, hi = n_preq - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].item0 <= it) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Points kernel, one thread per (instance, item): idx = inst * total_pitems + item.  pts: the point table as (k, f) pairs
// of 16 bytes, k an int64 and f a double; timing: [n_inst][n_timing][8] or null without a FIND request.
SPICEY_VAL_HD void spicey_val_points(int64_t idx, const SpiceyValDevPts *table, int32_t n_preq, int64_t total_pitems, const SpiceyValPoint *pts,
                                     const double *timing, int32_t n_timing, int64_t n_points, double dt, const double *a_v, int32_t n_v, const double *a_i,
                                     int32_t n_i, int32_t n_req, double *rows, int32_t out_stride) {
  const int64_t inst = idx / total_pitems, it = idx - inst * total_pitems;
  const SpiceyValDevPts q = table[spicey_val_find_req(table, n_preq, it)];
  const int64_t j = it - q.item0;
  double out[SPICEY_VAL_POINT_DOUBLES] = {-1.0, 0.0, 0.0, 0.0};
  int64_t k = -1;
  double f = 0.0;
  if (q.kind == 1) {
    const SpiceyValPoint p = pts[q.first + j];
    k = p.k;
    f = p.f;
  } else {
    const double *row = timing + (inst * (int64_t)n_timing + q.timing_row) * 8;
    const double kd = row[3];
    if (kd >= 0.0 && kd <= (double)(n_points - 2)) {
      k = (int64_t)kd;
      const double L = row[5];
      const int64_t nx = q.x_signal ? n_i : n_v;
      const double *bx = (q.x_signal ? a_i : a_v) + inst * n_points * nx;
      double a = bx[k * nx + q.x_col], b = bx[(k + 1) * nx + q.x_col];
      if (q.x_col_ref >= 0) {
        a = a - bx[k * nx + q.x_col_ref];
        b = b - bx[(k + 1) * nx + q.x_col_ref];
      }
      f = (L - a) / (b - a);
    }
  }
  if (k >= 0) {
    const int64_t n = q.signal ? n_i : n_v;
    const double *base = (q.signal ? a_i : a_v) + inst * n_points * n;
    if (q.col_ref < 0) {
      const double *pa = base + q.col;
      spicey_val_point(k, f, dt, [=](int64_t s) { return pa[s * n]; }, out);
    } else {
      const double *pa = base + q.col, *pb = base + q.col_ref;
      spicey_val_point(k, f, dt, [=](int64_t s) { return pa[s * n] - pb[s * n]; }, out);
    }
  }
  double *dst = rows + (inst * n_req + q.orig) * (int64_t)out_stride + j * SPICEY_VAL_POINT_DOUBLES;
  for (int c = 0; c < SPICEY_VAL_POINT_DOUBLES; c++) dst[c] = out[c];
}
