// power_exec.h — products of two signals over the step-major outputs of a transient run: the one definition of the
// reduction, used by the kernels of power.hip and by the CPU harness of tests/power_host (compiled without FMA contraction
// on both sides, so the two give the same bits).
//
// A request (SpiceyPowerReq, include/spicey_hip.h) names two factors a and b — each a column of out_v or out_i, minus a
// reference column (one rounded subtraction) when it has one —, a sign and an inclusive window of steps [from, to].  Per
// step p_k = a_k * b_k, one rounded product, negated when neg = 1.  Per (instance, request) SPICEY_POWER_ROW doubles come
// out:
//   {min_p, max_p, step_min, step_max, sum_p, first_p, last_p, sum_aa, sum_bb, first_a, last_a, first_b, last_b, 0, 0, 0}
// the extremes by the plain comparisons p < m and p > m in ascending step order (the FIRST occurrence is named, a NaN never
// replaces an extreme and does enter the sums), sum_aa / sum_bb with the square rounded first and then added.
//
// Combining order: the rule of measure_exec.h.  The window is cut into chunks of SPICEY_MEAS_CHUNK steps counted from ITS
// OWN first step; one thread walks a chunk in ascending step order from the chunk's first term (spicey_power_chunk); the
// chunk partials are combined in ascending chunk order by one thread (spicey_power_combine).  So a row is a function of
// the window's samples and the request alone: not of n_inst, the thread count, the grid or the other requests of the list.
#pragma once
#include <stdint.h>

#include "measure_exec.h"

#define SPICEY_POWER_LIVE 13  // the doubles of a row (and of a partial) that carry a value; the rest of the row is 0

// A validated request as the kernels read it: the table is sorted by (a_signal, a_col, b_signal, b_col), `orig` is the
// request's place in the caller's list (the row of the result it fills), `to` is resolved.
struct SpiceyPowerDevReq {
  int32_t a_signal, a_col, a_col_ref;
  int32_t b_signal, b_col, b_col_ref;
  int32_t neg, orig;
  int64_t from, to;
};

SPICEY_MEAS_HD int64_t spicey_power_chunks(const SpiceyPowerDevReq &q) { return (q.to - q.from) / SPICEY_MEAS_CHUNK + 1; }

// partial of (inst, chunk, sorted request): [n_inst][max_chunks][n_req][16] — neighbouring requests are neighbours in memory
SPICEY_MEAS_HD int64_t spicey_power_partial_index(int64_t inst, int64_t chunk, int64_t r, int64_t max_chunks, int64_t n_req) {
  return ((inst * max_chunks + chunk) * n_req + r) * SPICEY_POWER_ROW;
}

// One chunk of one request, steps in ascending order.  a(step) and b(step) are the factors' samples (the subtraction
// included).  out: the SPICEY_POWER_LIVE doubles of the partial, in the row's order.
template <class LoadA, class LoadB>
SPICEY_MEAS_HD void spicey_power_chunk(const SpiceyPowerDevReq &q, int64_t chunk, LoadA a, LoadB b, double *out) {
  const int64_t lo = q.from + chunk * SPICEY_MEAS_CHUNK;
  const int64_t hi = lo + SPICEY_MEAS_CHUNK - 1 < q.to ? lo + SPICEY_MEAS_CHUNK - 1 : q.to;
  const bool neg = q.neg != 0;
  const double a0 = a(lo), b0 = b(lo);
  const double ab0 = a0 * b0;
  const double p0 = neg ? -ab0 : ab0;
  double mn = p0, mx = p0, sum = p0, saa = a0 * a0, sbb = b0 * b0, lp = p0, la = a0, lb = b0;
  int64_t smn = lo, smx = lo;
  SPICEY_MEAS_UNROLL
  for (int64_t s = lo + 1; s <= hi; s++) {
    const double av = a(s), bv = b(s);
    const double ab = av * bv;
    const double p = neg ? -ab : ab;
    if (p < mn) { mn = p; smn = s; }
    if (p > mx) { mx = p; smx = s; }
    sum = sum + p;
    saa = saa + av * av;
    sbb = sbb + bv * bv;
    lp = p;
    la = av;
    lb = bv;
  }
  out[0] = mn; out[1] = mx; out[2] = (double)smn; out[3] = (double)smx;
  out[4] = sum; out[5] = p0; out[6] = lp; out[7] = saa; out[8] = sbb;
  out[9] = a0; out[10] = la; out[11] = b0; out[12] = lb;
}

// The request's chunk partials in ascending chunk order.  p(chunk) points at the doubles of that chunk's partial; out: the
// whole row, tail zeros included.
template <class Get>
SPICEY_MEAS_HD void spicey_power_combine(const SpiceyPowerDevReq &q, Get p, double *out) {
  const int64_t nc = spicey_power_chunks(q);
  const double *p0 = p(0);
  double r[SPICEY_POWER_LIVE];
  for (int j = 0; j < SPICEY_POWER_LIVE; j++) r[j] = p0[j];
  for (int64_t c = 1; c < nc; c++) {
    const double *pc = p(c);
    if (pc[0] < r[0]) { r[0] = pc[0]; r[2] = pc[2]; }
    if (pc[1] > r[1]) { r[1] = pc[1]; r[3] = pc[3]; }
    r[4] = r[4] + pc[4];
    r[6] = pc[6];
    r[7] = r[7] + pc[7];
    r[8] = r[8] + pc[8];
    r[10] = pc[10];
    r[12] = pc[12];
  }
  for (int j = 0; j < SPICEY_POWER_LIVE; j++) out[j] = r[j];
  for (int j = SPICEY_POWER_LIVE; j < SPICEY_POWER_ROW; j++) out[j] = 0.0;
}

// What thread `t` of the workgroup working on `tile` does in stage 1 (nothing when it falls off the request list or the
// request's chunks); g = spicey_meas_geom, the mapping of the measurement pass.  a_v / a_i: [n_inst][n_points][n_v | n_i].
// Two to four strided loads per step: a reference column is read only where the request has one.
SPICEY_MEAS_HD void spicey_power_stage1(const SpiceyMeasGeom &g, int64_t tile, int32_t t, const SpiceyPowerDevReq *table, int32_t n_req, int64_t n_points,
                                        const double *a_v, int32_t n_v, const double *a_i, int32_t n_i, double *partials) {
  const int64_t per_inst = g.r_tiles * g.c_tiles;
  const int64_t inst = tile / per_inst, rem = tile - inst * per_inst;
  const int64_t ct = rem / g.r_tiles, rt = rem - ct * g.r_tiles;
  const int64_t r = rt * g.rl + (t % g.rl), chunk = ct * g.cl + (t / g.rl);
  if (r >= n_req) return;
  const SpiceyPowerDevReq q = table[r];
  if (chunk >= spicey_power_chunks(q)) return;
  const int64_t na = q.a_signal ? n_i : n_v, nb = q.b_signal ? n_i : n_v;
  const double *base_a = (q.a_signal ? a_i : a_v) + inst * n_points * na;
  const double *base_b = (q.b_signal ? a_i : a_v) + inst * n_points * nb;
  const double *pa = base_a + q.a_col, *pb = base_b + q.b_col;
  double out[SPICEY_POWER_LIVE];
  const auto a1 = [=](int64_t s) { return pa[s * na]; };
  const auto b1 = [=](int64_t s) { return pb[s * nb]; };
  if (q.a_col_ref < 0 && q.b_col_ref < 0) {
    spicey_power_chunk(q, chunk, a1, b1, out);
  } else if (q.b_col_ref < 0) {
    const double *ra = base_a + q.a_col_ref;
    spicey_power_chunk(q, chunk, [=](int64_t s) { return pa[s * na] - ra[s * na]; }, b1, out);
  } else if (q.a_col_ref < 0) {
    const double *rb = base_b + q.b_col_ref;
    spicey_power_chunk(q, chunk, a1, [=](int64_t s) { return pb[s * nb] - rb[s * nb]; }, out);
  } else {
    const double *ra = base_a + q.a_col_ref, *rb = base_b + q.b_col_ref;
    spicey_power_chunk(q, chunk, [=](int64_t s) { return pa[s * na] - ra[s * na]; }, [=](int64_t s) { return pb[s * nb] - rb[s * nb]; }, out);
  }
  double *dst = partials + spicey_power_partial_index(inst, chunk, r, g.max_chunks, n_req);
  for (int j = 0; j < SPICEY_POWER_LIVE; j++) dst[j] = out[j];
}

// Stage 2, one thread per (instance, sorted request): idx = inst * n_req + r.
SPICEY_MEAS_HD void spicey_power_stage2(int64_t idx, const SpiceyPowerDevReq *table, int32_t n_req, int64_t max_chunks, const double *partials, double *rows) {
  const int64_t inst = idx / n_req, r = idx - inst * n_req;
  const SpiceyPowerDevReq q = table[r];
  double out[SPICEY_POWER_ROW];
  spicey_power_combine(q, [=](int64_t c) { return partials + spicey_power_partial_index(inst, c, r, max_chunks, n_req); }, out);
  double *dst = rows + (inst * n_req + q.orig) * SPICEY_POWER_ROW;
  for (int j = 0; j < SPICEY_POWER_ROW; j++) dst[j] = out[j];
}
