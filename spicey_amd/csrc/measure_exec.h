// measure_exec.h — waveform measurements over the step-major outputs of a transient run: the one definition of the
// reduction, used by the kernels of measure.hip and by the CPU harness of tests/measure_host (compiled without FMA
// contraction on both sides, so the two give the same bits).
//
// A request (SpiceyMeasReq, include/spicey_hip.h) names one signal x_k = a[inst][k][col] (minus a[inst][k][col_ref], one
// rounded subtraction, when col_ref >= 0) of out_v or out_i and an inclusive window of steps [from, to].  Per (instance,
// request) 8 doubles come out:
//   stats      {min, max, step_min, step_max, sum, sumsq, first, last}; the extremes by the plain comparisons x < m and
//              x > m in ascending step order, so step_min / step_max name the FIRST occurrence and a NaN sample never
//              becomes an extreme (it does enter the sums);
//   crossings  {count, t_first, t_last, 0, 0, 0, 0, 0} over the intervals (k, k + 1) with both ends in the window: a rise
//              is x_k < level && x_k+1 >= level, a fall x_k > level && x_k+1 <= level, at the time
//              ((double)k + (level - x_k) / (x_k+1 - x_k)) * dt; t_first = t_last = -1 without a crossing.
//
// Combining order (the fixed rule every result follows, whatever the launch looks like).  The window is cut into chunks of
// SPICEY_MEAS_CHUNK steps counted from ITS OWN first step: chunk c holds the steps from + c C .. min(from + (c + 1) C - 1,
// to).  One thread walks a chunk in ascending step order (spicey_meas_chunk); the chunk partials are combined in ascending
// chunk order by one thread (spicey_meas_combine).  The interval (k, k + 1) belongs to the chunk that holds k.  So a
// result is a function of the window's samples, dt and the request alone: not of n_inst, the thread count, the grid or the
// other requests of the list.
#pragma once
#include <stdint.h>

#include "../../include/spicey_hip.h"

#if defined(__HIPCC__)
#define SPICEY_MEAS_HD __host__ __device__ __forceinline__
#else
#define SPICEY_MEAS_HD inline
#endif
#if defined(__clang__)
#define SPICEY_MEAS_UNROLL _Pragma("unroll 8")
#else
#define SPICEY_MEAS_UNROLL
#endif

#define SPICEY_MEAS_CHUNK 256    // steps one thread reduces sequentially
#define SPICEY_MEAS_THREADS 256  // workgroup size of both kernels
#define SPICEY_MEAS_HEAD_ALIGN 256

// A validated request as the kernels read it: the table is sorted by (signal, col), `orig` is the request's place in the
// caller's list (the row of `meas` it fills), `to` is resolved.
struct SpiceyMeasDevReq {
  int32_t kind, signal, col, col_ref;
  int32_t dir, orig;
  int64_t from, to;
  double level;
};

// Stage 1 mapping.  A workgroup is `rl` requests wide (a power of two, the lanes of a wave first: neighbouring lanes read
// neighbouring columns) and `cl` chunks deep; few requests leave the lanes to the chunks.  Tiles are numbered instance-major,
// then chunk tile, then request tile; a workgroup takes the tiles blockIdx, blockIdx + gridDim, ...
struct SpiceyMeasGeom {
  int32_t rl, cl;
  int64_t r_tiles, c_tiles, max_chunks, tiles;
};

SPICEY_MEAS_HD SpiceyMeasGeom spicey_meas_geom(int32_t n_inst, int64_t n_points, int32_t n_req, int32_t threads) {
  SpiceyMeasGeom g;
  g.rl = 1;
  while (g.rl < n_req && g.rl < 64 && g.rl < threads) g.rl <<= 1;
  g.cl = threads / g.rl;
  g.max_chunks = (n_points + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK;
  g.r_tiles = ((int64_t)n_req + g.rl - 1) / g.rl;
  g.c_tiles = (g.max_chunks + g.cl - 1) / g.cl;
  g.tiles = (int64_t)n_inst * g.r_tiles * g.c_tiles;
  return g;
}

SPICEY_MEAS_HD int64_t spicey_meas_chunks(const SpiceyMeasDevReq &q) { return (q.to - q.from) / SPICEY_MEAS_CHUNK + 1; }

// partial of (inst, chunk, sorted request): [n_inst][max_chunks][n_req][8] — neighbouring requests are neighbours in memory
SPICEY_MEAS_HD int64_t spicey_meas_partial_index(int64_t inst, int64_t chunk, int64_t r, int64_t max_chunks, int64_t n_req) {
  return ((inst * max_chunks + chunk) * n_req + r) * 8;
}

// One chunk of one request, steps in ascending order.  x(step) is the signal's sample (the subtraction included).
template <class Load>
SPICEY_MEAS_HD void spicey_meas_chunk(const SpiceyMeasDevReq &q, int64_t chunk, double dt, Load x, double *out) {
  const int64_t lo = q.from + chunk * SPICEY_MEAS_CHUNK;
  const int64_t hi = lo + SPICEY_MEAS_CHUNK - 1 < q.to ? lo + SPICEY_MEAS_CHUNK - 1 : q.to;
  if (q.kind == 0) {
    const double x0 = x(lo);
    double mn = x0, mx = x0, sum = x0, sq = x0 * x0, last = x0;
    int64_t smn = lo, smx = lo;
    SPICEY_MEAS_UNROLL
    for (int64_t s = lo + 1; s <= hi; s++) {
      const double v = x(s);
      if (v < mn) { mn = v; smn = s; }
      if (v > mx) { mx = v; smx = s; }
      sum = sum + v;
      sq = sq + v * v;
      last = v;
    }
    out[0] = mn; out[1] = mx; out[2] = (double)smn; out[3] = (double)smx;
    out[4] = sum; out[5] = sq; out[6] = x0; out[7] = last;
  } else {
    const int64_t kend = hi < q.to ? hi : q.to - 1;  // (the interval that leaves the chunk is this chunk's)
    const bool rise = q.dir >= 0, fall = q.dir <= 0;
    const double level = q.level;
    double cnt = 0.0, tf = -1.0, tl = -1.0;
    double a = x(lo);
    SPICEY_MEAS_UNROLL
    for (int64_t k = lo; k <= kend; k++) {
      const double b = x(k + 1);
      const bool hit = (rise && a < level && b >= level) || (fall && a > level && b <= level);
      if (hit) {
        const double t = ((double)k + (level - a) / (b - a)) * dt;
        if (cnt == 0.0) tf = t;
        tl = t;
        cnt = cnt + 1.0;
      }
      a = b;
    }
    out[0] = cnt; out[1] = tf; out[2] = tl;
    out[3] = 0.0; out[4] = 0.0; out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
  }
}

// The request's chunk partials in ascending chunk order.  p(chunk) points at the 8 doubles of that chunk.
template <class Get>
SPICEY_MEAS_HD void spicey_meas_combine(const SpiceyMeasDevReq &q, Get p, double *out) {
  const int64_t nc = spicey_meas_chunks(q);
  const double *p0 = p(0);
  double r[8];
  for (int j = 0; j < 8; j++) r[j] = p0[j];
  for (int64_t c = 1; c < nc; c++) {
    const double *pc = p(c);
    if (q.kind == 0) {
      if (pc[0] < r[0]) { r[0] = pc[0]; r[2] = pc[2]; }
      if (pc[1] > r[1]) { r[1] = pc[1]; r[3] = pc[3]; }
      r[4] = r[4] + pc[4];
      r[5] = r[5] + pc[5];
      r[7] = pc[7];
    } else if (pc[0] > 0.0) {
      if (r[0] == 0.0) r[1] = pc[1];
      r[2] = pc[2];
      r[0] = r[0] + pc[0];
    }
  }
  for (int j = 0; j < 8; j++) out[j] = r[j];
}

// What thread `t` of the workgroup working on `tile` does in stage 1 (nothing when it falls off the request list or the
// request's chunks).  a_v / a_i: [n_inst][n_points][n_v | n_i].
SPICEY_MEAS_HD void spicey_meas_stage1(const SpiceyMeasGeom &g, int64_t tile, int32_t t, const SpiceyMeasDevReq *table, int32_t n_req, int64_t n_points,
                                       double dt, const double *a_v, int32_t n_v, const double *a_i, int32_t n_i, double *partials) {
  const int64_t per_inst = g.r_tiles * g.c_tiles;
  const int64_t inst = tile / per_inst, rem = tile - inst * per_inst;
  const int64_t ct = rem / g.r_tiles, rt = rem - ct * g.r_tiles;
  const int64_t r = rt * g.rl + (t % g.rl), chunk = ct * g.cl + (t / g.rl);
  if (r >= n_req) return;
  const SpiceyMeasDevReq q = table[r];
  if (chunk >= spicey_meas_chunks(q)) return;
  const int64_t n = q.signal ? n_i : n_v;
  const double *base = (q.signal ? a_i : a_v) + inst * n_points * n;
  double out[8];
  if (q.col_ref < 0) {
    const double *pa = base + q.col;
    spicey_meas_chunk(q, chunk, dt, [=](int64_t s) { return pa[s * n]; }, out);
  } else {
    const double *pa = base + q.col, *pb = base + q.col_ref;
    spicey_meas_chunk(q, chunk, dt, [=](int64_t s) { return pa[s * n] - pb[s * n]; }, out);
  }
  double *dst = partials + spicey_meas_partial_index(inst, chunk, r, g.max_chunks, n_req);
  for (int j = 0; j < 8; j++) dst[j] = out[j];
}

// Stage 2, one thread per (instance, sorted request): idx = inst * n_req + r.
SPICEY_MEAS_HD void spicey_meas_stage2(int64_t idx, const SpiceyMeasDevReq *table, int32_t n_req, int64_t max_chunks, const double *partials, double *meas) {
  const int64_t inst = idx / n_req, r = idx - inst * n_req;
  const SpiceyMeasDevReq q = table[r];
  double out[8];
  spicey_meas_combine(q, [=](int64_t c) { return partials + spicey_meas_partial_index(inst, c, r, max_chunks, n_req); }, out);
  double *dst = meas + (inst * n_req + q.orig) * 8;
  for (int j = 0; j < 8; j++) dst[j] = out[j];
}

// ---- host side: validation, the sorted table, the workspace layout ---------------------------------------------------
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

// `b` bytes rounded up to the alignment of a workspace's regions (all reduction passes)
inline int64_t spicey_meas_align(int64_t b) { return (b + SPICEY_MEAS_HEAD_ALIGN - 1) / SPICEY_MEAS_HEAD_ALIGN * SPICEY_MEAS_HEAD_ALIGN; }

// bytes of the request table at the head of the workspace
inline int64_t spicey_meas_head_bytes(int32_t n_req) { return spicey_meas_align((int64_t)n_req * (int64_t)sizeof(SpiceyMeasDevReq)); }

// table | partials; -1 for arguments no launch accepts
inline int64_t spicey_meas_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  if (n_inst <= 0 || n_points <= 0 || n_req <= 0) return -1;
  const int64_t max_chunks = (n_points + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK;
  return spicey_meas_head_bytes(n_req) + (int64_t)n_inst * max_chunks * (int64_t)n_req * 8 * (int64_t)sizeof(double);
}

// Checks every request and builds the kernels' table; false + `err` for a request no launch accepts.
inline bool spicey_meas_plan(const SpiceyMeasReq *reqs, int32_t n_req, int64_t n_points, int32_t n_v, int32_t n_i, bool have_i,
                             std::vector<SpiceyMeasDevReq> &table, std::string &err) {
  char buf[200];
  table.clear();
  if (!reqs || n_req <= 0) { err = "measure: n_req must be >= 1 and the request list not null"; return false; }
  if (n_points <= 0) { err = "measure: n_points must be >= 1"; return false; }
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyMeasReq &q = reqs[i];
    const char *what = nullptr;
    if (q.kind != 0 && q.kind != 1) what = "unknown kind (0 = stats, 1 = crossings)";
    else if (q.signal != 0 && q.signal != 1) what = "unknown signal (0 = out_v, 1 = out_i)";
    else if (q.dir != 0 && q.dir != 1 && q.dir != -1) what = "unknown dir (+1 rise, -1 fall, 0 either)";
    else if (q.signal == 1 && !have_i) what = "signal = 1 without a current buffer";
    const int64_t to = q.step_to == -1 ? n_points - 1 : q.step_to;
    if (!what) {
      const int32_t n = q.signal ? n_i : n_v;
      if (q.col < 0 || q.col >= n || q.col_ref < -1 || q.col_ref >= n) what = "column out of range";
      else if (q.step_from < 0 || to < 0 || to >= n_points || q.step_from > to) what = "window outside [0, n_points) or step_from > step_to";
    }
    if (what) {
      snprintf(buf, sizeof(buf), "measure: request %d: %s", (int)i, what);
      err = buf;
      table.clear();
      return false;
    }
    table.push_back(SpiceyMeasDevReq{q.kind, q.signal, q.col, q.col_ref, q.dir, i, q.step_from, to, q.level});
  }
  std::stable_sort(table.begin(), table.end(), [](const SpiceyMeasDevReq &a, const SpiceyMeasDevReq &b) {
    return a.signal != b.signal ? a.signal < b.signal : a.col < b.col;
  });
  return true;
}
