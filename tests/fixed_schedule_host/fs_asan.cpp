// tests/fixed_schedule_host/fs_asan.cpp — a stand-alone program (TEST INFRASTRUCTURE ONLY) for the address and undefined-behaviour
// sanitizers, linked with harness.cpp: the plan of a handle as spicey_create makes it, with and without
// SPICEY_NO_FIXED_SCHEDULE, the predicate on the resident layout as built and with one condition broken at a time, and 8 steps
// of the emulated packed kernel in its fixed schedule against the fused form whose loop decides its schedule in every step.
// The workspace of every workgroup is a heap block of exactly spicey_lds_bytes bytes, the parameter record with the two
// tables behind it and every result, source and iteration-count buffer a heap block of exactly the planned size.  Chains of
// 511 nodes (the smallest that takes the form), of 1000 nodes (the benchmark's length) and of 1018 (the largest); chains of
// 766 and 1022 nodes, which take the fuse but stream a second phase and are refused; and one of 100 nodes that no plan
// fuses.  Built and run by `make asan`; no GPU and no python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_fshost_run(const SpiceyDesc *d, int32_t form, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *out_v,
                                     double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags, int64_t *info8,
                                     int32_t *err4, int64_t *solves_out);
extern "C" int32_t spicey_fshost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out8);
extern "C" int32_t spicey_fshost_predicate(const SpiceyDesc *d, int32_t T, int64_t *out8);

namespace {

// V1 n1 0, then per stage k: R n_k n_k+1, C and D between n_k+1 and ground
struct Chain {
  int n, ni;
  std::vector<int32_t> Rn1, Rn2, Cn1, Cn2, Vn1, Vn2, Dp, Dm;
  std::vector<double> Rv, Cv, Cvp, Dis, Dn, Dvd;
  SpiceyDesc d{};
  Chain(int n_, int ni_) : n(n_), ni(ni_) {
    for (int k = 1; k < n; k++) {
      Rn1.push_back(k); Rn2.push_back(k + 1);
      Cn1.push_back(k + 1); Cn2.push_back(0);
      Dp.push_back(k + 1); Dm.push_back(0);
    }
    Vn1.push_back(1); Vn2.push_back(0);
    for (int g = 0; g < ni; g++) {
      for (size_t k = 0; k < Rn1.size(); k++) Rv.push_back(100.0 * (1.0 + 0.01 * g + 0.001 * (double)(k % 7)));
      for (size_t k = 0; k < Cn1.size(); k++) { Cv.push_back(1e-9 * (1.0 + 0.02 * g)); Cvp.push_back(0.0); }
      for (size_t k = 0; k < Dp.size(); k++) { Dis.push_back(1e-14 * (1.0 + 0.1 * g)); Dn.push_back(1.0 + 0.05 * (double)(k % 3)); Dvd.push_back(0.0); }
    }
    d.abi_version = SPICEY_ABI_VERSION; d.n_nodes = n; d.n_inst = ni;
    d.nR = (int32_t)Rn1.size(); d.nC = (int32_t)Cn1.size(); d.nL = 0; d.nV = 1; d.nS = 0; d.nD = (int32_t)Dp.size();
    d.R_n1 = Rn1.data(); d.R_n2 = Rn2.data(); d.R_val = Rv.data();
    d.C_n1 = Cn1.data(); d.C_n2 = Cn2.data(); d.C_val = Cv.data(); d.C_vprev = Cvp.data();
    d.V_n1 = Vn1.data(); d.V_n2 = Vn2.data();
    d.D_np = Dp.data(); d.D_nm = Dm.data(); d.D_is = Dis.data(); d.D_n = Dn.data(); d.D_vdprev = Dvd.data();
    d.n_out = 0; d.out_nodes = nullptr;
  }
};

int fail(const char *what) { fprintf(stderr, "fs_asan: %s\n", what); return 1; }

const int T = 512;

struct Out {
  std::vector<double> v, i, Cv, Dv, src;
  std::vector<int32_t> it;
  int64_t info[8] = {};
  int64_t solves = 0;
  int32_t rc = 0;
};

Out run(const Chain &ch, int form, int64_t steps, int flags) {
  Out o;
  const int nCur = ch.d.nR + ch.d.nC + ch.d.nV + ch.d.nD;
  o.src.resize((size_t)(steps + 1));
  for (size_t s = 0; s < o.src.size(); s++) o.src[s] = (s & 2) ? 3.0 : -3.0;
  o.v.assign((size_t)ch.ni * (steps + 1) * ch.d.n_nodes, 0.0);
  o.i.assign((size_t)ch.ni * (steps + 1) * nCur, 0.0);
  o.it.assign((size_t)ch.ni * (steps + 1), 0);
  o.Cv = ch.Cvp; o.Dv = ch.Dvd;
  int32_t err4[4] = {0, 0, 0, 0};
  o.rc = spicey_fshost_run(&ch.d, form, T, steps, 1e-6, o.src.data(), 0, o.v.data(), o.i.data(), o.it.data(), o.Cv.data(), nullptr, o.Dv.data(), nullptr, flags, o.info, err4,
                           &o.solves);
  return o;
}

bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

// the form the plan of a handle takes, with the knob or without: 1 / 0, -1 on an error
int planned(const Chain &ch, bool knob, int64_t steps) {
  if (knob) setenv("SPICEY_NO_FIXED_SCHEDULE", "1", 1);
  else unsetenv("SPICEY_NO_FIXED_SCHEDULE");
  SpiceyOptions opt{};
  opt.geometry = 2; opt.want_currents = 1;
  int64_t p[8];
  const int32_t rc = spicey_fshost_plan(&ch.d, &opt, 256, steps, p);
  unsetenv("SPICEY_NO_FIXED_SCHEDULE");
  if (rc != SPICEY_OK) return -1;
  printf("plan of chain(%d) x %d, knob %d: fixed_schedule %lld stamp_fuse %lld packed %lld fresh %lld threads %lld -> fixed %lld fused %lld\n", ch.n, ch.ni, (int)knob,
         (long long)p[0], (long long)p[1], (long long)p[3], (long long)p[4], (long long)p[5], (long long)p[6], (long long)p[7]);
  if (!p[3] || !p[4]) return -1;  // (not the packed fresh build)
  if (knob && p[7] != p[1]) return -1;  // (the knob leaves the fuse alone)
  return (int)p[6];
}

int one(int n, int ni, int64_t steps, int takes) {
  Chain ch(n, ni);
  const int with_knob = planned(ch, true, steps), without = planned(ch, false, steps);
  if (with_knob != 0) return fail("the knob does not keep the loop that decides its schedule in every step");
  if (without != takes) return fail(takes ? "the plan does not take the fixed schedule" : "the plan takes the fixed schedule where its conditions fail");
  int64_t pr[8];
  if (spicey_fshost_predicate(&ch.d, T, pr) != 0) return fail("the predicate's harness failed");
  printf("chain(%d): predicate %lld, broken one at a time: %lld %lld %lld %lld %lld %lld\n", n, (long long)pr[0], (long long)pr[1], (long long)pr[2], (long long)pr[3], (long long)pr[4],
         (long long)pr[5], (long long)pr[6]);
  if (pr[0] != takes) return fail("the predicate and the plan disagree");
  for (int k = 1; k <= 6; k++)
    if (pr[k] > 0) return fail("the predicate accepts a layout the written-out loop cannot run");
  if (!takes) return run(ch, 1, 2, 0).rc != 0 ? 0 : fail("the harness runs the fixed schedule where the plan would not");
  const Out off = run(ch, 0, steps, 0);
  if (off.rc) return fail("the fused run failed");
  const Out on = run(ch, 1, steps, 2), rev = run(ch, 1, steps, 3), own = run(ch, 1, steps, 2 | 4);
  printf("chain(%d) x %d, %lld steps: rc %d %d %d %d, %lld solves\n", n, ni, (long long)steps, off.rc, on.rc, rev.rc, own.rc, (long long)on.solves);
  if (on.rc || rev.rc || own.rc) return fail("a run of the fixed schedule failed");
  for (const Out *o : {&on, &rev, &own})
    if (!same(off.v, o->v) || !same(off.i, o->i) || off.it != o->it || !same(off.Cv, o->Cv) || !same(off.Dv, o->Dv) || off.solves != o->solves) return fail("the form on and off differ");
  double sum = 0.0;
  for (double v : on.v) sum += v;
  for (double v : on.i) sum += v;
  if (!(sum == sum)) return fail("NaN in the result");
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad |= one(100, 2, 8, 0);
  bad |= one(511, 3, 8, 1);
  bad |= one(1000, 2, 8, 1);
  bad |= one(1018, 1, 8, 1);
  bad |= one(766, 1, 8, 0);
  bad |= one(1022, 1, 8, 0);
  printf(bad ? "fs_asan: FAILED\n" : "fs_asan: ok\n");
  return bad;
}
