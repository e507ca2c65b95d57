// fourier_exec.h — harmonics of a transient's waveforms (what SPICE calls .four): the one definition of the reduction, used
// by the kernels of fourier.hip and by the CPU harness of tests/fourier_host (compiled without FMA contraction on both
// sides, so the two give the same bits).
//
// A request (SpiceyFourReq, include/spicey_hip.h) names one signal x_s = a[inst][s][col] (minus a[inst][s][col_ref], one
// rounded subtraction, when col_ref >= 0) of out_v or out_i, a fundamental f0, a harmonic count n_harm and the window of
// the N = step_to - step_from steps step_from .. step_to - 1.  Per (instance, request) 1 + 2 n_harm doubles come out:
//   {C0, C1, S1, ..., CH, SH},  C0 = sum x_s,  C_h = sum x_s c(h, s),  S_h = sum x_s s(h, s)
// with s the ABSOLUTE step (phases refer to t = 0) and c / s the twiddles of spicey_four_twiddle below — a HOST function:
// the device never evaluates a sine, it reads the table the host built (one per basis (f0, step_from, step_to), as wide
// as the largest n_harm among the basis' requests).
//
// Combining order (the rule of measure_exec.h).  The window is cut into chunks of SPICEY_MEAS_CHUNK steps counted from ITS
// OWN first step; one thread walks a chunk in ascending step order with 1 + 2 H running sums that start at 0.0, every
// product and every sum rounded on its own (spicey_four_chunk); the chunk partials are added in ascending chunk order,
// starting from chunk 0's (spicey_four_stage2).  A harmonic's sums do not see the other harmonics, so a row is a function
// of the window's samples, dt and the request alone: not of n_inst, the launch, the other requests or the basis' width.
#pragma once
#include <stdint.h>

#include "measure_exec.h"  // SPICEY_MEAS_CHUNK, SPICEY_MEAS_THREADS, SPICEY_MEAS_HEAD_ALIGN: one chunking for every reduction

#define SPICEY_FOUR_HD SPICEY_MEAS_HD
#define SPICEY_FOUR_WAVE 64  // requests a stage 1 tile is wide: the lanes of one wave

// A validated request as the kernels read it: the table is sorted by (basis, signal, col); `orig` is the request's place in
// the caller's list (the row of the result it fills), `rr` its place among its basis' requests.
struct SpiceyFourDevReq {
  int32_t signal, col, col_ref, n_harm;
  int32_t orig, basis, rr, pad;
};

// One basis (f0, from, to): its H = largest n_harm, its twiddles [to - from][H][2] = {c, s} at tw_off doubles into the
// twiddle area, its partials [chunks][1 + 2 H][n_req] at p_off doubles into an instance's partials (neighbouring requests
// are neighbours in memory), and its stage 1 tiles: r_tiles x c_tiles of them from tile_first on, request tile fastest.
struct SpiceyFourBasis {
  int64_t from, to, chunks;
  int64_t tw_off, p_off, tile_first, c_tiles;
  int32_t H, n_req, r_first, r_tiles;
};

SPICEY_FOUR_HD int64_t spicey_four_partial_index(const SpiceyFourBasis &b, int64_t chunk, int32_t j, int32_t rr) {
  return ((chunk * (1 + 2 * b.H) + j) * b.n_req + rr);
}

// One chunk of one request with the basis' H harmonics: steps lo .. hi - 1 in ascending order, tw = the basis' twiddles
// at step lo, x(step) the signal's sample (the subtraction included, once per step).  Sum j goes to dst[j * stride].
template <int H, class Load>
SPICEY_FOUR_HD void spicey_four_chunk(int64_t lo, int64_t hi, const double *tw, Load x, double *dst, int64_t stride) {
  double c0 = 0.0, C[H], S[H];
#if defined(__clang__)
#pragma unroll
#endif
  for (int h = 0; h < H; h++) C[h] = S[h] = 0.0;
#if defined(__clang__)
#pragma unroll 2
#endif
  for (int64_t s = lo; s < hi; s++) {
    const double v = x(s);
    const double *t = tw + (s - lo) * (2 * H);
    c0 = c0 + v;
#if defined(__clang__)
#pragma unroll
#endif
    for (int h = 0; h < H; h++) {
      C[h] = C[h] + v * t[2 * h];
      S[h] = S[h] + v * t[2 * h + 1];
    }
  }
  dst[0] = c0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int h = 0; h < H; h++) {
    dst[(1 + 2 * h) * stride] = C[h];
    dst[(2 + 2 * h) * stride] = S[h];
  }
}

// (the running sums are indexed by constants only, so they stay in registers: one instance of the loop per width)
template <class Load>
SPICEY_FOUR_HD void spicey_four_chunk_h(int32_t H, int64_t lo, int64_t hi, const double *tw, Load x, double *dst, int64_t stride) {
  switch (H) {
#define SPICEY_FOUR_CASE(n) case n: spicey_four_chunk<n>(lo, hi, tw, x, dst, stride); break;
    SPICEY_FOUR_CASE(1) SPICEY_FOUR_CASE(2) SPICEY_FOUR_CASE(3) SPICEY_FOUR_CASE(4) SPICEY_FOUR_CASE(5) SPICEY_FOUR_CASE(6)
    SPICEY_FOUR_CASE(7) SPICEY_FOUR_CASE(8) SPICEY_FOUR_CASE(9) SPICEY_FOUR_CASE(10) SPICEY_FOUR_CASE(11) SPICEY_FOUR_CASE(12)
    SPICEY_FOUR_CASE(13) SPICEY_FOUR_CASE(14) SPICEY_FOUR_CASE(15) SPICEY_FOUR_CASE(16)
#undef SPICEY_FOUR_CASE
    default: break;
  }
}

// Stage 1 mapping.  A tile is SPICEY_FOUR_WAVE requests of ONE basis wide (`rl` = min(64, threads): the lanes of a wave
// take neighbouring requests, so they read neighbouring columns of one row) and `cl` = threads / rl chunks deep: the waves
// of a workgroup spread over chunks.  A wave therefore sits at one step of one basis' table at a time — `slot` (which of the
// tile's chunks: wave-uniform) and everything derived from it, the twiddle address included, is the same in all its lanes.
// Tiles are numbered instance-major, then basis, then chunk tile, then request tile; a workgroup takes the tiles blockIdx,
// blockIdx + gridDim, ...  `lane` = t % rl, `slot` = t / rl.  a_v / a_i: [n_inst][n_points][n_v | n_i].
SPICEY_FOUR_HD void spicey_four_stage1(int64_t tile, int32_t lane, int32_t slot, int32_t rl, int32_t cl, int64_t tiles_per_inst,
                                       const SpiceyFourDevReq *table, const SpiceyFourBasis *bases, int32_t n_basis, const double *tw, int64_t n_points,
                                       const double *a_v, int32_t n_v, const double *a_i, int32_t n_i, double *partials, int64_t partials_per_inst) {
  const int64_t inst = tile / tiles_per_inst, rem = tile - inst * tiles_per_inst;
  int32_t bi = 0;
  while (bi + 1 < n_basis && bases[bi + 1].tile_first <= rem) bi++;
  const SpiceyFourBasis b = bases[bi];
  const int64_t tb = rem - b.tile_first;
  const int64_t ct = tb / b.r_tiles, rt = tb - ct * b.r_tiles;
  const int64_t chunk = ct * cl + slot;
  const int64_t rr = rt * rl + lane;
  if (chunk >= b.chunks || rr >= b.n_req) return;
  const SpiceyFourDevReq q = table[b.r_first + rr];
  const int64_t lo = b.from + chunk * SPICEY_MEAS_CHUNK;
  const int64_t hi = lo + SPICEY_MEAS_CHUNK < b.to ? lo + SPICEY_MEAS_CHUNK : b.to;
  const double *twc = tw + b.tw_off + chunk * SPICEY_MEAS_CHUNK * (2 * (int64_t)b.H);
  const int64_t n = q.signal ? n_i : n_v;
  const double *base = (q.signal ? a_i : a_v) + inst * n_points * n;
  double *dst = partials + inst * partials_per_inst + b.p_off + spicey_four_partial_index(b, chunk, 0, (int32_t)rr);
  if (q.col_ref < 0) {
    const double *pa = base + q.col;
    spicey_four_chunk_h(b.H, lo, hi, twc, [=](int64_t s) { return pa[s * n]; }, dst, (int64_t)b.n_req);
  } else {
    const double *pa = base + q.col, *pb = base + q.col_ref;
    spicey_four_chunk_h(b.H, lo, hi, twc, [=](int64_t s) { return pa[s * n] - pb[s * n]; }, dst, (int64_t)b.n_req);
  }
}

// Stage 2, one thread per (instance, sorted request, element of the caller's row): idx = (inst * n_req + r) * out_stride + j.
// The elements past the request's 1 + 2 n_harm are 0.
SPICEY_FOUR_HD void spicey_four_stage2(int64_t idx, const SpiceyFourDevReq *table, const SpiceyFourBasis *bases, int32_t n_req, int32_t out_stride,
                                       const double *partials, int64_t partials_per_inst, double *out) {
  const int64_t ir = idx / out_stride;
  const int32_t j = (int32_t)(idx - ir * out_stride);
  const int64_t inst = ir / n_req, r = ir - inst * n_req;
  const SpiceyFourDevReq q = table[r];
  double v = 0.0;
  if (j < 1 + 2 * q.n_harm) {
    const SpiceyFourBasis b = bases[q.basis];
    const double *p = partials + inst * partials_per_inst + b.p_off;
    v = p[spicey_four_partial_index(b, 0, j, q.rr)];
    for (int64_t c = 1; c < b.chunks; c++) v = v + p[spicey_four_partial_index(b, c, j, q.rr)];
  }
  out[(inst * n_req + q.orig) * out_stride + j] = v;
}

// ---- host side: the twiddles, validation, the sorted table, the workspace layout ----------------------------------------
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// c(h, s), s(h, s): the turn count h s f0 dt reduced to [0, 1) before it meets 2 pi, so the argument of cos / sin stays small
// however late the window is.  f0dt = f0 * dt, one rounded product.  (No a * b + c in here: nothing a compiler could fuse.)
inline void spicey_four_twiddle(int32_t h, int64_t s, double f0dt, double *c, double *sn) {
  double r = (double)((int64_t)h * s) * f0dt;
  r = r - std::floor(r);
  const double a = (2.0 * 3.141592653589793) * r;
  // (cos and sin proper: a compiler that sees both calls on one value makes them one sincos call, and this libm's sincos
  // does not always return cos' and sin's bits — the copy through a volatile keeps the two calls apart)
  volatile double a_again = a;
  *c = std::cos(a);
  *sn = std::sin(a_again);
}

// Everything a launch needs, from the request list alone: sorted table, bases, twiddles, sizes.
struct SpiceyFourPlan {
  std::vector<SpiceyFourDevReq> table;
  std::vector<SpiceyFourBasis> bases;
  std::vector<double> f0;  // per basis
  int32_t max_harm = 0;
  int64_t tw_doubles = 0, partials_per_inst = 0, tiles_per_inst = 0;
  int32_t rl = 0, cl = 0;
  // head of the workspace: table | bases | twiddles, each aligned; then the partials
  int64_t off_bases = 0, off_tw = 0, head_bytes = 0;
  int64_t workspace_bytes(int32_t n_inst) const { return head_bytes + (int64_t)n_inst * partials_per_inst * (int64_t)sizeof(double); }
};

// The tiles of a launch with workgroups of `threads` threads (a power of two).
inline void spicey_four_geom(SpiceyFourPlan &p, int32_t threads) {
  p.rl = threads < SPICEY_FOUR_WAVE ? threads : SPICEY_FOUR_WAVE;
  p.cl = threads / p.rl;
  int64_t t = 0;
  for (SpiceyFourBasis &b : p.bases) {
    b.r_tiles = (b.n_req + p.rl - 1) / p.rl;
    b.c_tiles = (b.chunks + p.cl - 1) / p.cl;
    b.tile_first = t;
    t += (int64_t)b.r_tiles * b.c_tiles;
  }
  p.tiles_per_inst = t;
}

// What the request list alone decides — windows, harmonic counts, fundamentals — checked, and the layout built from it
// (spicey_fourier_workspace_bytes needs no more).  false + `err` for a list no launch accepts.
inline bool spicey_four_layout(const SpiceyFourReq *reqs, int32_t n_req, int64_t n_points, SpiceyFourPlan &p, std::string &err) {
  char buf[200];
  p = SpiceyFourPlan();
  if (!reqs || n_req <= 0) { err = "fourier: n_req must be >= 1 and the request list not null"; return false; }
  if (n_points <= 0) { err = "fourier: n_points must be >= 1"; return false; }
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyFourReq &q = reqs[i];
    const int64_t to = q.step_to == -1 ? n_points - 1 : q.step_to;
    const char *what = nullptr;
    if (q.n_harm < 1 || q.n_harm > SPICEY_FOUR_MAX_HARM) what = "n_harm outside 1..16";
    else if (!(q.f0 > 0.0) || !std::isfinite(q.f0)) what = "f0 must be finite and > 0";
    else if (q.step_from < 0 || to < 0 || to >= n_points || q.step_from >= to) what = "window outside [0, n_points) or step_from >= step_to";
    if (what) {
      snprintf(buf, sizeof(buf), "fourier: request %d: %s", (int)i, what);
      err = buf;
      return false;
    }
    int32_t bi = 0;
    for (; bi < (int32_t)p.bases.size(); bi++)
      if (memcmp(&p.f0[bi], &q.f0, sizeof(double)) == 0 && p.bases[bi].from == q.step_from && p.bases[bi].to == to) break;
    if (bi == (int32_t)p.bases.size()) {
      SpiceyFourBasis b{};
      b.from = q.step_from;
      b.to = to;
      b.chunks = (to - q.step_from + SPICEY_MEAS_CHUNK - 1) / SPICEY_MEAS_CHUNK;
      p.bases.push_back(b);
      p.f0.push_back(q.f0);
    }
    SpiceyFourBasis &b = p.bases[bi];
    b.H = std::max(b.H, q.n_harm);
    b.n_req++;
    p.max_harm = std::max(p.max_harm, q.n_harm);
    p.table.push_back(SpiceyFourDevReq{q.signal, q.col, q.col_ref, q.n_harm, i, bi, 0, 0});
  }
  std::stable_sort(p.table.begin(), p.table.end(), [](const SpiceyFourDevReq &a, const SpiceyFourDevReq &b) {
    return a.basis != b.basis ? a.basis < b.basis : a.signal != b.signal ? a.signal < b.signal : a.col < b.col;
  });
  int32_t r = 0;
  for (SpiceyFourBasis &b : p.bases) {
    b.r_first = r;
    for (int32_t k = 0; k < b.n_req; k++) p.table[r + k].rr = k;
    r += b.n_req;
    b.tw_off = p.tw_doubles;
    p.tw_doubles += (b.to - b.from) * 2 * b.H;
    b.p_off = p.partials_per_inst;
    p.partials_per_inst += b.chunks * (1 + 2 * b.H) * b.n_req;
  }
  p.off_bases = spicey_meas_align((int64_t)p.table.size() * (int64_t)sizeof(SpiceyFourDevReq));
  p.off_tw = p.off_bases + spicey_meas_align((int64_t)p.bases.size() * (int64_t)sizeof(SpiceyFourBasis));
  p.head_bytes = p.off_tw + spicey_meas_align(p.tw_doubles * (int64_t)sizeof(double));
  spicey_four_geom(p, SPICEY_MEAS_THREADS);
  return true;
}

// table | bases | twiddles | partials; -1 for arguments no launch accepts
inline int64_t spicey_four_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyFourReq *reqs, int32_t n_req) {
  SpiceyFourPlan p;
  std::string err;
  if (n_inst <= 0 || !spicey_four_layout(reqs, n_req, n_points, p, err)) return -1;
  return p.workspace_bytes(n_inst);
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing): counts, buffers, the request
// list, dt and Nyquist, the row stride, the workspace size.  true: `p` holds the launch's tables.
inline bool spicey_four_judge(int32_t n_inst, int64_t n_points, double dt, bool have_v, int32_t n_v, bool have_i, int32_t n_i, const SpiceyFourReq *reqs,
                              int32_t n_req, bool have_out, int32_t out_stride, int64_t work_bytes, SpiceyFourPlan &p, std::string &err) {
  char buf[224];
  if (n_inst <= 0 || n_v < 0 || n_i < 0 || !have_out) { err = "fourier: bad arguments (n_inst >= 1, result and workspace buffers)"; return false; }
  if (!(dt > 0.0) || !std::isfinite(dt)) { err = "fourier: dt must be finite and > 0"; return false; }
  if (!spicey_four_layout(reqs, n_req, n_points, p, err)) return false;
  for (int32_t i = 0; i < n_req; i++) {
    const SpiceyFourReq &q = reqs[i];
    const char *what = nullptr;
    if (q.signal != 0 && q.signal != 1) what = "unknown signal (0 = out_v, 1 = out_i)";
    else if (q.signal == 1 && !have_i) what = "signal = 1 without a current buffer";
    else {
      const int32_t n = q.signal ? n_i : (have_v ? n_v : 0);
      if (q.col < 0 || q.col >= n || q.col_ref < -1 || q.col_ref >= n) what = "column out of range";
      else if ((double)q.n_harm * (q.f0 * dt) > 0.5) what = "n_harm f0 dt > 0.5: the highest harmonic is above Nyquist";
    }
    if (what) {
      snprintf(buf, sizeof(buf), "fourier: request %d: %s", (int)i, what);
      err = buf;
      return false;
    }
  }
  if (out_stride < 1 + 2 * p.max_harm) {
    snprintf(buf, sizeof(buf), "fourier: out_stride %d is too small, %d needed (1 + 2 n_harm)", (int)out_stride, (int)(1 + 2 * p.max_harm));
    err = buf;
    return false;
  }
  const int64_t need = p.workspace_bytes(n_inst);
  if (work_bytes < need) {
    snprintf(buf, sizeof(buf), "fourier: workspace of %lld bytes is too small, %lld needed (spicey_fourier_workspace_bytes)", (long long)work_bytes, (long long)need);
    err = buf;
    return false;
  }
  return true;
}

// The head of the workspace as one block of host memory: table | bases | twiddles (built here, by spicey_four_twiddle).
inline void spicey_four_head(const SpiceyFourPlan &p, double dt, std::vector<unsigned char> &head) {
  head.assign((size_t)p.head_bytes, 0);
  memcpy(head.data(), p.table.data(), p.table.size() * sizeof(SpiceyFourDevReq));
  memcpy(head.data() + p.off_bases, p.bases.data(), p.bases.size() * sizeof(SpiceyFourBasis));
  double *tw = (double *)(head.data() + p.off_tw);
  for (size_t bi = 0; bi < p.bases.size(); bi++) {
    const SpiceyFourBasis &b = p.bases[bi];
    const double f0dt = p.f0[bi] * dt;
    double *t = tw + b.tw_off;
    for (int64_t s = b.from; s < b.to; s++)
      for (int32_t h = 1; h <= b.H; h++, t += 2) spicey_four_twiddle(h, s, f0dt, t, t + 1);
  }
}
