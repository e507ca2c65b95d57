// Stand-alone check of the edge-timing harness under the host sanitizers (-fsanitize=address,undefined; see the Makefile):
// the harness entry (harness.cpp over timing_exec.h: the index-heavy code the kernels run) on constructed cases and a few
// seeded pool shapes, against a straightforward scan written out here — every crossing of the window collected into a
// vector, then the occurrence picked.  Exit status 0 only if every row agrees bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_tim_host_chunk(void);
extern "C" int32_t spicey_tim_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                       const SpiceyTimingReq *reqs, int32_t n_req, double *out, int64_t work_bytes, int32_t threads, int64_t grid, char *err,
                                       int32_t err_cap);

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }
  int32_t below(int32_t n) { return (int32_t)(next() % (uint32_t)n); }
};

struct Waves {
  int32_t n_inst, n_v, n_i;
  int64_t n_points;
  std::vector<double> v, i;
  double at(const SpiceyTimingEdge &e, int32_t inst, int64_t s) const {
    const std::vector<double> &a = e.signal ? i : v;
    const int64_t n = e.signal ? n_i : n_v;
    const double x = a[(size_t)((inst * n_points + s) * n + e.col)];
    return e.col_ref >= 0 ? x - a[(size_t)((inst * n_points + s) * n + e.col_ref)] : x;
  }
};

double level_of(const Waves &w, const SpiceyTimingEdge &e, int32_t inst) {
  if (e.level_kind == 0) return e.level;
  const int64_t b1 = e.base_to == -1 ? w.n_points - 1 : e.base_to;
  double lo = w.at(e, inst, e.base_from), hi = lo;
  if (e.level_kind == 1) {
    for (int64_t s = e.base_from; s <= b1; s++) {
      const double x = w.at(e, inst, s);
      if (x < lo) lo = x;
      if (x > hi) hi = x;
    }
  } else {
    hi = w.at(e, inst, b1);
  }
  const double span = hi - lo;
  const double part = e.level * span;
  return lo + part;
}

// k, t, count of edge e among the crossings of the intervals k0 .. k1 - 1
void find(const Waves &w, const SpiceyTimingEdge &e, int32_t inst, double L, int64_t k0, int64_t k1, double dt, double *k, double *t, double *cnt) {
  std::vector<int64_t> ks;
  for (int64_t s = k0; s < k1; s++) {
    const double a = w.at(e, inst, s), b = w.at(e, inst, s + 1);
    if ((e.dir >= 0 && a < L && b >= L) || (e.dir <= 0 && a > L && b <= L)) ks.push_back(s);
  }
  const int64_t m = e.n >= 1 ? e.n - 1 : (int64_t)ks.size() + e.n;
  *cnt = (double)ks.size();
  *k = *t = -1.0;
  if (m < 0 || m >= (int64_t)ks.size()) return;
  const double a = w.at(e, inst, ks[(size_t)m]), b = w.at(e, inst, ks[(size_t)m] + 1);
  *k = (double)ks[(size_t)m];
  *t = ((double)ks[(size_t)m] + (L - a) / (b - a)) * dt;
}

void scan(const Waves &w, const SpiceyTimingReq &q, int32_t inst, double dt, double *row) {
  const double init[8] = {-1.0, -1.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0};
  memcpy(row, init, sizeof(init));
  const int64_t s1 = q.step_to == -1 ? w.n_points - 1 : q.step_to;
  int64_t k0 = q.step_from;
  bool search = true;
  if (q.has_trig) {
    row[2] = level_of(w, q.trig, inst);
    find(w, q.trig, inst, row[2], q.step_from, s1, dt, row + 0, row + 1, row + 6);
    if (q.targ_from_trig) { search = row[0] >= 0.0; k0 = (int64_t)row[0]; }
  }
  row[5] = level_of(w, q.targ, inst);
  if (search) find(w, q.targ, inst, row[5], k0, s1, dt, row + 3, row + 4, row + 7);
}

Waves waves(int32_t n_inst, int64_t n_points, int32_t n_v, int32_t n_i, uint64_t seed) {
  Waves w{n_inst, n_v, n_i, n_points, {}, {}};
  Rng r{seed};
  auto fill = [&](std::vector<double> &a, int32_t n) {
    a.resize((size_t)(n_inst * n_points * n));
    for (double &x : a) x = r.below(10) < 7 ? (r.below(9) - 4) / 4.0 : (r.below(1980) - 990) / 1000.0;  // nine values a quarter apart, or anything
  };
  fill(w.v, n_v);
  fill(w.i, n_i);
  return w;
}

SpiceyTimingEdge edge(int32_t signal, int32_t col, int32_t col_ref, int32_t dir, int32_t n, int32_t kind, int64_t b0, int64_t b1, double level) {
  return SpiceyTimingEdge{signal, col, col_ref, dir, n, kind, b0, b1, level};
}

int failures = 0;

void check(const char *what, const Waves &w, const std::vector<SpiceyTimingReq> &reqs, double dt, int32_t threads, int64_t grid) {
  std::vector<double> got((size_t)w.n_inst * reqs.size() * 8, 7.0);
  char err[256] = "";
  const int32_t rc = spicey_tim_host_run(w.n_inst, w.n_points, dt, w.v.data(), w.n_v, w.i.data(), w.n_i, reqs.data(), (int32_t)reqs.size(), got.data(), -1, threads,
                                         grid, err, 256);
  if (rc != SPICEY_OK) { printf("FAIL %s: refused: %s\n", what, err); failures++; return; }
  int bad = 0;
  for (int32_t inst = 0; inst < w.n_inst; inst++)
    for (size_t r = 0; r < reqs.size(); r++) {
      double want[8];
      scan(w, reqs[r], inst, dt, want);
      if (memcmp(want, &got[((size_t)inst * reqs.size() + r) * 8], sizeof(want)) != 0 && bad++ < 3)
        printf("FAIL %s: instance %d request %zu: k_targ %g / %g, n_targ %g / %g\n", what, (int)inst, r, got[((size_t)inst * reqs.size() + r) * 8 + 3], want[3],
               got[((size_t)inst * reqs.size() + r) * 8 + 7], want[7]);
    }
  if (bad) failures++;
  else printf("ok   %s: %d x %zu rows\n", what, (int)w.n_inst, reqs.size());
}

std::vector<SpiceyTimingReq> pool(const Waves &w, int32_t count, uint64_t seed) {
  Rng r{seed};
  const int64_t C = spicey_tim_host_chunk(), last = w.n_points - 1;
  std::vector<int64_t> marks;
  for (int64_t s : {(int64_t)0, (int64_t)1, (int64_t)37, C - 1, C, C + 1, 2 * C, last / 2, last - 1, last})
    if (s >= 0 && s <= last) marks.push_back(s);
  auto one_edge = [&]() {
    const int32_t sig = r.below(2), n = sig ? w.n_i : w.n_v, kind = r.below(3);
    const int64_t a = marks[(size_t)r.below((int32_t)marks.size())], b = marks[(size_t)r.below((int32_t)marks.size())];
    const double abs_l[4] = {0.25, 0.1, -0.5, 0.0}, rel_l[6] = {0.0, 0.25, 0.5, 0.75, 1.0, 1.25};
    int32_t nn = r.below(8) - 3;
    if (nn <= 0) nn -= 1;  // -4 .. -1, 1 .. 4
    return edge(sig, r.below(n), r.below(3) == 2 ? r.below(n) : -1, r.below(3) - 1, nn, kind, a < b ? a : b, r.below(4) == 0 ? -1 : (a < b ? b : a),
                kind == 0 ? abs_l[r.below(4)] : rel_l[r.below(6)]);
  };
  std::vector<SpiceyTimingReq> reqs;
  while ((int32_t)reqs.size() < count) {
    int64_t a = marks[(size_t)r.below((int32_t)marks.size())], b = marks[(size_t)r.below((int32_t)marks.size())];
    if (a == b) continue;
    if (a > b) { const int64_t t = a; a = b; b = t; }
    const int32_t has_trig = r.below(2);
    reqs.push_back(SpiceyTimingReq{a, b == last && r.below(2) ? -1 : b, has_trig, has_trig ? r.below(2) : 0, one_edge(), one_edge()});
  }
  return reqs;
}

}  // namespace

int main() {
  const double dt = 1e-6;
  const int64_t C = spicey_tim_host_chunk();
  // constructed: a ramp-and-back signal in column 0, its scaled copies in the other instances, a flat column 1
  {
    Waves w{3, 2, 1, 2 * C + 5, {}, {}};
    w.v.assign((size_t)(w.n_inst * w.n_points * 2), 0.0);
    w.i.assign((size_t)(w.n_inst * w.n_points), 0.0);
    for (int32_t inst = 0; inst < 3; inst++)
      for (int64_t s = 0; s < w.n_points; s++) {
        double x = (double)(s % 8 < 4 ? s % 8 : 8 - s % 8);  // 0 1 2 3 4 3 2 1 ...
        if (s == C - 1) x = 0.0;
        if (s == C) x = 4.0;  // a rise through every level in interval (C - 1, C): chunk 0's
        w.v[(size_t)((inst * w.n_points + s) * 2)] = x * (double)(1 << inst);
        w.v[(size_t)((inst * w.n_points + s) * 2 + 1)] = 2.5;
        w.i[(size_t)(inst * w.n_points + s)] = 4.0 - x;  // falls where column 0 rises, in the same interval
      }
    std::vector<SpiceyTimingReq> q;
    const SpiceyTimingEdge none = edge(0, 0, -1, 1, 1, 0, 0, 0, 0.0);
    for (int32_t n : {1, 2, -1, -2, 1000, -1000})
      for (int32_t kind : {0, 1, 2})
        for (int32_t dir : {1, -1, 0}) {
          q.push_back(SpiceyTimingReq{0, -1, 0, 0, none, edge(0, 0, -1, dir, n, kind, 0, -1, kind ? 0.5 : 1.5)});
          q.push_back(SpiceyTimingReq{C - 1, C, 0, 0, none, edge(0, 0, -1, dir, n, kind, 3, C + 9, kind ? 0.5 : 1.5)});  // the one interval (C - 1, C)
          q.push_back(SpiceyTimingReq{3, 2 * C + 1, 1, 1, edge(0, 0, -1, dir, n, 1, 0, -1, 0.75), edge(1, 0, -1, -dir, 1, 1, 0, -1, 0.5)});
          q.push_back(SpiceyTimingReq{3, 2 * C + 1, 1, 0, edge(0, 0, -1, dir, 1, 1, 0, -1, 0.5), edge(0, 0, -1, dir, n, 1, 0, -1, 0.5)});
          q.push_back(SpiceyTimingReq{0, -1, 1, 1, edge(0, 0, -1, dir, -1, 1, 0, -1, 0.5), edge(0, 0, -1, dir, n, 1, 0, -1, 0.5)});  // trig in the last crossing
          q.push_back(SpiceyTimingReq{0, -1, 1, 1, edge(0, 1, -1, dir, n, kind, 0, -1, 0.5), edge(0, 0, 1, dir, n, kind, 5, 5, 0.5)});  // a flat trig
        }
    check("constructed", w, q, dt, 256, 0);
    check("constructed, 32 threads, 3 workgroups", w, q, dt, 32, 3);
  }
  int k = 0;
  for (int64_t n_points : {(int64_t)2, C - 1, C, C + 1, 3 * C + 7})
    for (int32_t n_v : {1, 65}) {
      const Waves w = waves(3, n_points, n_v, 5, 100 + (uint64_t)k);
      char name[64];
      snprintf(name, sizeof(name), "pool n_points %lld n_v %d", (long long)n_points, (int)n_v);
      const std::vector<SpiceyTimingReq> q = pool(w, 150, 7 + (uint64_t)k);
      check(name, w, q, dt, k % 2 ? 64 : 256, k % 3);
      k++;
    }
  printf(failures ? "selftest: %d group(s) FAILED\n" : "selftest: all groups agree\n", failures);
  return failures ? 1 : 0;
}
