// timing_exec.h — edge timing over the step-major outputs of a transient run (the n-th crossing of a level, the delay from
// one edge to another): the one definition of the reduction, used by the kernels of timing.hip and by the CPU harness of
// tests/timing_host (compiled without FMA contraction on both sides, so the two give the same bits).
//
// An edge (SpiceyTimingEdge, include/spicey_hip.h) names one signal x_k exactly as SpiceyMeasReq does, a direction, an
// occurrence n != 0 and a level: absolute, or L = lo + level * (hi - lo) — the product, the difference and the sum each
// rounded on its own — with (lo, hi) the signal's (min, max) or (first, last) over the edge's base window in THAT instance.
// A crossing is the measurement pass's: a rise is x_k < L && x_k+1 >= L, a fall x_k > L && x_k+1 <= L, in interval k, at
// the time ((double)k + (L - x_k) / (x_k+1 - x_k)) * dt.  A request (SpiceyTimingReq) has a window [from, to] — the
// intervals from .. to - 1 —, a targ edge and an optional trig edge.  The trig is searched in the window; so is the targ,
// unless targ_from_trig = 1: then in the window's intervals k >= k_trig.  n >= 1 is the n-th crossing of the search range
// in ascending k, n <= -1 the |n|-th from its end.  Every selection is by the integer k; no interpolated times are compared.
// Per (instance, request) 8 doubles come out: {k_trig, t_trig, L_trig, k_targ, t_targ, L_targ, n_trig, n_targ}.
//
// Every field has one value in any evaluation order (integer counts; min / max / first / last; two fixed formulas), so a
// row is a function of the window's samples, dt and the request alone: not of n_inst, the grid, the workgroup size or the
// other requests of the list.  The mapping: intervals are cut into chunks of SPICEY_MEAS_CHUNK counted from the window's
// first step, interval k belongs to the chunk that holds k.  Stage 1: one thread per (instance, edge, chunk) resolves the
// level, walks the chunk in step order and leaves its crossing count as an int32 in [inst][chunk][edge].  Stage 2: one
// thread per (instance, request) adds the counts in ascending chunk order until it knows which chunk holds the wanted
// crossing, walks that one chunk again and takes the crossing's k and time; for targ_from_trig the chunk that holds k_trig
// is walked once more for its crossings with k >= k_trig before the later chunks' counts are added.
#pragma once
#include <stdint.h>

#include "measure_exec.h"  // SPICEY_MEAS_CHUNK, SPICEY_MEAS_THREADS, SPICEY_MEAS_HEAD_ALIGN, SpiceyMeasDevReq, spicey_meas_geom

#define SPICEY_TIM_HD SPICEY_MEAS_HD

// A validated edge as the kernels read it: the table is sorted by (signal, col); `base` is the row of the base results
// the level is resolved from (-1: absolute), from / to the window of the edge's request (to resolved).
struct SpiceyTimDevEdge {
  int32_t signal, col, col_ref, dir;
  int32_t n, level_kind, base, pad;
  int64_t from, to;
  double level;
};

// A request as stage 2 reads it: the sorted places of its edges (e_trig = -1: none) and the row of the result it fills.
// The table is sorted by e_targ: where neighbouring requests ask for neighbouring columns and their wanted crossings fall
// into the same chunk, neighbouring threads walk neighbouring addresses; trig walks and requests whose chunks differ do not.
struct SpiceyTimDevReq {
  int32_t e_trig, e_targ, targ_from_trig, orig;
};

SPICEY_TIM_HD int64_t spicey_tim_chunks(const SpiceyTimDevEdge &e) { return (e.to - e.from + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK; }

// count of (inst, chunk, sorted edge): [n_inst][max_chunks][n_edge] — neighbouring edges are neighbours in memory
SPICEY_TIM_HD int64_t spicey_tim_count_index(int64_t inst, int64_t chunk, int64_t e, int64_t max_chunks, int64_t n_edge) {
  return (inst * max_chunks + chunk) * n_edge + e;
}

// The level of edge e in one instance; base_rows: that instance's [n_base][8] stats rows {min, max, ., ., ., ., first, last}.
SPICEY_TIM_HD double spicey_tim_level(const SpiceyTimDevEdge &e, const double *base_rows) {
  if (e.level_kind == 0) return e.level;
  const double *b = base_rows + (int64_t)e.base * 8;
  const double lo = e.level_kind == 1 ? b[0] : b[6], hi = e.level_kind == 1 ? b[1] : b[7];
  const double span = hi - lo;
  const double part = e.level * span;
  return lo + part;
}

// One chunk of one edge, intervals in ascending order: the number of crossings with k >= kmin.  With m >= 1 the m-th of
// them is also looked for: its k goes to *k_hit and its time to *t_hit (both left alone when the chunk has fewer).
template <class Load>
SPICEY_TIM_HD int32_t spicey_tim_walk(const SpiceyTimDevEdge &e, double L, int64_t chunk, int64_t kmin, int32_t m, double dt, Load x, int64_t *k_hit,
                                      double *t_hit) {
  int64_t lo = e.from + chunk * SPICEY_MEAS_CHUNK;
  const int64_t hi = lo + SPICEY_MEAS_CHUNK - 1 < e.to - 1 ? lo + SPICEY_MEAS_CHUNK - 1 : e.to - 1;  // last interval of the chunk
  if (lo < kmin) lo = kmin;
  if (lo > hi) return 0;
  const bool rise = e.dir >= 0, fall = e.dir <= 0;
  int32_t cnt = 0;
  double a = x(lo);
  SPICEY_MEAS_UNROLL
  for (int64_t k = lo; k <= hi; k++) {
    const double b = x(k + 1);
    const bool hit = (rise && a < L && b >= L) || (fall && a > L && b <= L);
    if (hit) {
      cnt++;
      if (cnt == m) {
        *k_hit = k;
        *t_hit = ((double)k + (L - a) / (b - a)) * dt;
      }
    }
    a = b;
  }
  return cnt;
}

// What thread `t` of the workgroup working on `tile` does in stage 1 (nothing when it falls off the edge list or the edge's
// chunks); the geometry is the measurement pass's with edges in the place of requests.  a_v / a_i: [n_inst][n_points][n_v | n_i];
// base_out: [n_inst][n_base][8].
SPICEY_TIM_HD void spicey_tim_stage1(const SpiceyMeasGeom &g, int64_t tile, int32_t t, const SpiceyTimDevEdge *edges, int32_t n_edge, int32_t n_base,
                                     int64_t n_points, const double *a_v, int32_t n_v, const double *a_i, int32_t n_i, const double *base_out,
                                     int32_t *counts) {
  const int64_t per_inst = g.r_tiles * g.c_tiles;
  const int64_t inst = tile / per_inst, rem = tile - inst * per_inst;
  const int64_t ct = rem / g.r_tiles, rt = rem - ct * g.r_tiles;
  const int64_t r = rt * g.rl + (t % g.rl), chunk = ct * g.cl + (t / g.rl);
  if (r >= n_edge) return;
  const SpiceyTimDevEdge e = edges[r];
  if (chunk >= spicey_tim_chunks(e)) return;
  const double L = spicey_tim_level(e, base_out + inst * (int64_t)n_base * 8);
  const int64_t n = e.signal ? n_i : n_v;
  const double *base = (e.signal ? a_i : a_v) + inst * n_points * n;
  int64_t k = 0;
  double tt = 0.0;
  int32_t cnt;
  if (e.col_ref < 0) {
    const double *pa = base + e.col;
    cnt = spicey_tim_walk(e, L, chunk, e.from, 0, 0.0, [=](int64_t s) { return pa[s * n]; }, &k, &tt);
  } else {
    const double *pa = base + e.col, *pb = base + e.col_ref;
    cnt = spicey_tim_walk(e, L, chunk, e.from, 0, 0.0, [=](int64_t s) { return pa[s * n] - pb[s * n]; }, &k, &tt);
  }
  counts[spicey_tim_count_index(inst, chunk, r, g.max_chunks, n_edge)] = cnt;
}

// The occurrence e.n of edge `ei` among its crossings with k >= kmin (kmin >= e.from): *k_out / *t_out = the selected
// interval and time or -1, *n_out = the number of crossings in that range.  cnt(chunk) is the chunk's stage 1 count.
template <class Load, class Count>
SPICEY_TIM_HD void spicey_tim_select(const SpiceyTimDevEdge &e, double L, int64_t kmin, double dt, Load x, Count cnt, double *k_out, double *t_out,
                                     double *n_out) {
  const int64_t nc = spicey_tim_chunks(e);
  const int64_t c0 = (kmin - e.from) / SPICEY_MEAS_CHUNK;
  int64_t k = -1;
  double t = -1.0;
  // (the chunk the range starts in counts in full when the range starts with it, else by a walk of its own)
  const int64_t first = kmin == e.from + c0 * SPICEY_MEAS_CHUNK ? (int64_t)cnt(c0) : (int64_t)spicey_tim_walk(e, L, c0, kmin, 0, dt, x, &k, &t);
  int64_t total = first;
  for (int64_t c = c0 + 1; c < nc; c++) total += cnt(c);
  const int64_t m = e.n >= 1 ? (int64_t)e.n : total + (int64_t)e.n + 1;  // the occurrence counted from the range's start
  if (m >= 1 && m <= total) {
    int64_t c = c0, before = 0, here = first;
    while (before + here < m) {
      before += here;
      c++;
      here = cnt(c);
    }
    (void)spicey_tim_walk(e, L, c, kmin, (int32_t)(m - before), dt, x, &k, &t);
  }
  *k_out = (double)k;
  *t_out = t;
  *n_out = (double)total;
}

// Stage 2, one thread per (instance, sorted request): idx = inst * n_req + r.
SPICEY_TIM_HD void spicey_tim_stage2(int64_t idx, const SpiceyTimDevReq *reqs, int32_t n_req, const SpiceyTimDevEdge *edges, int32_t n_edge, int32_t n_base,
                                     int64_t max_chunks, int64_t n_points, double dt, const double *a_v, int32_t n_v, const double *a_i, int32_t n_i,
                                     const double *base_out, const int32_t *counts, double *out) {
  const int64_t inst = idx / n_req, r = idx - inst * n_req;
  const SpiceyTimDevReq q = reqs[r];
  const double *brow = base_out + inst * (int64_t)n_base * 8;
  double res[8] = {-1.0, -1.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0};
  int64_t kmin = -1;
  bool search_targ = true;
  for (int pass = 0; pass < 2; pass++) {
    const int32_t ei = pass == 0 ? q.e_trig : q.e_targ;
    if (ei < 0) continue;
    const SpiceyTimDevEdge e = edges[ei];
    const double L = spicey_tim_level(e, brow);
    double *o = res + 3 * pass;
    o[2] = L;
    if (pass == 1 && !search_targ) continue;
    const int64_t from = pass == 1 && kmin >= 0 ? kmin : e.from;
    const int64_t n = e.signal ? n_i : n_v;
    const double *base = (e.signal ? a_i : a_v) + inst * n_points * n;
    auto cnt = [=](int64_t c) { return counts[spicey_tim_count_index(inst, c, ei, max_chunks, n_edge)]; };
    if (e.col_ref < 0) {
      const double *pa = base + e.col;
      spicey_tim_select(e, L, from, dt, [=](int64_t s) { return pa[s * n]; }, cnt, o, o + 1, res + 6 + pass);
    } else {
      const double *pa = base + e.col, *pb = base + e.col_ref;
      spicey_tim_select(e, L, from, dt, [=](int64_t s) { return pa[s * n] - pb[s * n]; }, cnt, o, o + 1, res + 6 + pass);
    }
    if (pass == 0 && q.targ_from_trig) {
      if (o[0] < 0.0) search_targ = false;
      else kmin = (int64_t)o[0];
    }
  }
  double *dst = out + (inst * n_req + q.orig) * 8;
  for (int j = 0; j < 8; j++) dst[j] = res[j];
}

// ---- host side: validation, the sorted tables, the workspace layout --------------------------------------------------
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

// Everything a launch needs, from the request list alone: the sorted edge and request tables, the base windows as stats
// requests of the measurement pass (distinct (signal, col, col_ref, base_from, base_to), sorted like its tables), sizes.
struct SpiceyTimPlan {
  std::vector<SpiceyTimDevEdge> edges;
  std::vector<SpiceyTimDevReq> reqs;
  std::vector<SpiceyMeasDevReq> bases;
  int64_t max_chunks = 0;
  // workspace: edges | requests (the head, one upload) | base rows [n_inst][n_base][8] | the measurement pass's own workspace
  // for the bases (n_base > 0) | counts [n_inst][max_chunks][n_edge] int32
  int64_t off_reqs = 0, head_bytes = 0;
  int64_t off_base_out() const { return head_bytes; }
  int64_t off_base_work(int32_t n_inst) const { return head_bytes + spicey_meas_align((int64_t)n_inst * (int64_t)bases.size() * 8 * (int64_t)sizeof(double)); }
  int64_t off_counts(int32_t n_inst, int64_t n_points) const {
    const int64_t w = bases.empty() ? 0 : spicey_meas_workspace_bytes(n_inst, n_points, (int32_t)bases.size());
    return off_base_work(n_inst) + spicey_meas_align(w);
  }
  int64_t workspace_bytes(int32_t n_inst, int64_t n_points) const {
    return off_counts(n_inst, n_points) + spicey_meas_align((int64_t)n_inst * max_chunks * (int64_t)edges.size() * (int64_t)sizeof(int32_t));
  }
};

// Checks every request and builds the tables; false + `err` for a list no launch accepts.  check_cols = false leaves out
// what only the buffers decide (column ranges, the current buffer): spicey_timing_workspace_bytes needs no more.
inline bool spicey_tim_plan(const SpiceyTimingReq *reqs, int32_t n_req, int64_t n_points, bool check_cols, int32_t n_v, int32_t n_i, bool have_i,
                            SpiceyTimPlan &p, std::string &err) {
  char buf[224];
  p = SpiceyTimPlan();
  if (!reqs || n_req <= 0) { err = "timing: n_req must be >= 1 and the request list not null"; return false; }
  if (n_points <= 0) { err = "timing: n_points must be >= 1"; return false; }
  struct Tmp { SpiceyTimDevEdge e; int32_t req, role; };
  std::vector<Tmp> tmp;
  std::vector<SpiceyMeasDevReq> bases;  // in order of first use; `orig` = that order
  std::map<std::tuple<int32_t, int32_t, int32_t, int64_t, int64_t>, int32_t> base_of;  // (signal, col, col_ref, from, to) -> its place in `bases`
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyTimingReq &q = reqs[i];
    const int64_t to = q.step_to == -1 ? n_points - 1 : q.step_to;
    const char *what = nullptr, *who = "";
    if (q.has_trig != 0 && q.has_trig != 1) what = "has_trig must be 0 or 1";
    else if (q.targ_from_trig != 0 && q.targ_from_trig != 1) what = "targ_from_trig must be 0 or 1";
    else if (q.targ_from_trig && !q.has_trig) what = "targ_from_trig without has_trig";
    else if (q.step_from < 0 || to < 0 || to >= n_points || q.step_from > to) what = "window outside [0, n_points) or step_from > step_to";
    else if (q.step_from == to) what = "a window of one point has no interval";
    for (int32_t role = q.has_trig ? 0 : 1; role < 2 && !what; role++) {
      const SpiceyTimingEdge &e = role == 0 ? q.trig : q.targ;
      who = role == 0 ? "trig: " : "targ: ";
      const int64_t bto = e.base_to == -1 ? n_points - 1 : e.base_to;
      if (e.signal != 0 && e.signal != 1) what = "unknown signal (0 = out_v, 1 = out_i)";
      else if (e.dir != 0 && e.dir != 1 && e.dir != -1) what = "unknown dir (+1 rise, -1 fall, 0 either)";
      else if (e.level_kind < 0 || e.level_kind > 2) what = "unknown level_kind (0 absolute, 1 of min/max, 2 of first/last)";
      else if (e.n == 0) what = "n must not be 0";
      else if (!std::isfinite(e.level)) what = "the level (or fraction) must be finite";
      else if (e.level_kind != 0 && (e.base_from < 0 || bto < 0 || bto >= n_points || e.base_from > bto)) what = "base window outside [0, n_points) or base_from > base_to";
      else if (check_cols) {
        const int32_t n = e.signal ? n_i : n_v;
        if (e.signal == 1 && !have_i) what = "signal = 1 without a current buffer";
        else if (e.col < 0 || e.col >= n || e.col_ref < -1 || e.col_ref >= n) what = "column out of range";
      }
      if (what) break;
      int32_t bi = -1;
      if (e.level_kind != 0) {
        const auto ins = base_of.emplace(std::make_tuple(e.signal, e.col, e.col_ref, e.base_from, bto), (int32_t)bases.size());
        bi = ins.first->second;
        if (ins.second) bases.push_back(SpiceyMeasDevReq{0, e.signal, e.col, e.col_ref, 0, bi, e.base_from, bto, 0.0});
      }
      tmp.push_back(Tmp{SpiceyTimDevEdge{e.signal, e.col, e.col_ref, e.dir, e.n, e.level_kind, bi, 0, q.step_from, to, e.level}, i, role});
    }
    if (what) {
      snprintf(buf, sizeof(buf), "timing: request %d: %s%s", (int)i, who, what);
      err = buf;
      return false;
    }
  }
  std::stable_sort(tmp.begin(), tmp.end(), [](const Tmp &a, const Tmp &b) { return a.e.signal != b.e.signal ? a.e.signal < b.e.signal : a.e.col < b.e.col; });
  p.reqs.assign((size_t)n_req, SpiceyTimDevReq{-1, -1, 0, 0});
  for (int32_t k = 0; k < (int32_t)tmp.size(); k++) {
    p.edges.push_back(tmp[k].e);
    SpiceyTimDevReq &r = p.reqs[tmp[k].req];
    (tmp[k].role == 0 ? r.e_trig : r.e_targ) = k;
  }
  for (int32_t i = 0; i < n_req; i++) { p.reqs[i].targ_from_trig = reqs[i].targ_from_trig; p.reqs[i].orig = i; }
  std::stable_sort(p.reqs.begin(), p.reqs.end(), [](const SpiceyTimDevReq &a, const SpiceyTimDevReq &b) { return a.e_targ < b.e_targ; });
  // (the measurement pass writes row `orig` of its result and wants its table sorted by (signal, col): `orig` stays the
  // order of first use, which is what SpiceyTimDevEdge::base names)
  p.bases = bases;
  std::stable_sort(p.bases.begin(), p.bases.end(), [](const SpiceyMeasDevReq &a, const SpiceyMeasDevReq &b) { return a.signal != b.signal ? a.signal < b.signal : a.col < b.col; });
  p.max_chunks = (n_points + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK;
  p.off_reqs = spicey_meas_align((int64_t)p.edges.size() * (int64_t)sizeof(SpiceyTimDevEdge));
  p.head_bytes = p.off_reqs + spicey_meas_align((int64_t)p.reqs.size() * (int64_t)sizeof(SpiceyTimDevReq));
  return true;
}

// edges | requests | base rows | base workspace | counts; -1 for arguments no launch accepts
inline int64_t spicey_tim_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyTimingReq *reqs, int32_t n_req) {
  SpiceyTimPlan p;
  std::string err;
  if (n_inst <= 0 || !spicey_tim_plan(reqs, n_req, n_points, false, 0, 0, false, p, err)) return -1;
  return p.workspace_bytes(n_inst, n_points);
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing): counts, buffers, dt, the
// request list, the workspace size.  true: `p` holds the launch's tables.
inline bool spicey_tim_judge(int32_t n_inst, int64_t n_points, double dt, bool have_v, int32_t n_v, bool have_i, int32_t n_i, const SpiceyTimingReq *reqs,
                             int32_t n_req, bool have_out, int64_t work_bytes, SpiceyTimPlan &p, std::string &err) {
  char buf[224];
  if (n_inst <= 0 || n_v < 0 || n_i < 0 || !have_out) { err = "timing: bad arguments (n_inst >= 1, result and workspace buffers)"; return false; }
  if (!(dt > 0.0) || !std::isfinite(dt)) { err = "timing: dt must be finite and > 0"; return false; }
  if (!spicey_tim_plan(reqs, n_req, n_points, true, have_v ? n_v : 0, n_i, have_i, p, err)) return false;
  const int64_t need = p.workspace_bytes(n_inst, n_points);
  if (work_bytes < need) {
    snprintf(buf, sizeof(buf), "timing: workspace of %lld bytes is too small, %lld needed (spicey_timing_workspace_bytes)", (long long)work_bytes, (long long)need);
    err = buf;
    return false;
  }
  return true;
}

// The head of the workspace as one block of host memory: edges | requests.
inline void spicey_tim_head(const SpiceyTimPlan &p, std::vector<unsigned char> &head) {
  head.assign((size_t)p.head_bytes, 0);
  memcpy(head.data(), p.edges.data(), p.edges.size() * sizeof(SpiceyTimDevEdge));
  memcpy(head.data() + p.off_reqs, p.reqs.data(), p.reqs.size() * sizeof(SpiceyTimDevReq));
}
