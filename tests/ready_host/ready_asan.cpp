// tests/ready_host/ready_asan.cpp — a stand-alone program (TEST INFRASTRUCTURE ONLY) for the address and undefined-behaviour
// sanitizers, linked with harness.cpp: the prologue's rebasing of the record, source and iteration-count pointers
// (tran_pt.h: spicey_pt_rebase_ready), the hot reads of Z and of the early fetch through them, the reads inside Z's
// last-step branch and inside the inductor loop, and the launch's decision (launch_plan.cpp: spicey_ready_run).  Every
// buffer a rebased pointer reaches into is a heap allocation of exactly the planned size — the record ni x 2 x T x 5
// doubles, the source table ni x (steps + 1) x nV, the results ni x (steps + 1) x row, the counts ni x (steps + 1) — so a
// base that is one instance or one row off lands in a red zone.  Every circuit runs with and without ready arguments and
// must give the same bytes.  Built and run by `make asan`; no GPU and no python involved.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_rahost_run(const SpiceyDesc *d, int32_t ready, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *zpar,
                                     double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags,
                                     uint32_t *table, int64_t *info8);
extern "C" void spicey_rahost_words(int32_t *out8);
extern "C" int32_t spicey_rahost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out8);

namespace {

// V1 n1 0 (and `nv` - 1 further sources on nodes of their own, each through a resistor into the chain), then per stage k:
// R n_k n_k+1 — `ind`: every fifth stage an inductor instead —, C and D between n_k+1 and ground
struct Chain {
  int n, ni, nv;
  std::vector<int32_t> Rn1, Rn2, Cn1, Cn2, Ln1, Ln2, Vn1, Vn2, Dp, Dm;
  std::vector<double> Rv, Cv, Cvp, Lv, Lip, Dis, Dn, Dvd;
  SpiceyDesc d{};
  Chain(int n_, int ni_, int nv_, bool ind) : n(n_), ni(ni_), nv(nv_) {
    for (int k = 1; k < n; k++) {
      if (ind && k % 5 == 0) { Ln1.push_back(k); Ln2.push_back(k + 1); }
      else { Rn1.push_back(k); Rn2.push_back(k + 1); }
      Cn1.push_back(k + 1); Cn2.push_back(0);
      Dp.push_back(k + 1); Dm.push_back(0);
    }
    Vn1.push_back(1); Vn2.push_back(0);
    for (int v = 1; v < nv; v++) {  // source v on node n + v, a resistor from there into the chain
      Vn1.push_back(n + v); Vn2.push_back(0);
      Rn1.push_back(n + v); Rn2.push_back(1 + (n - 1) * v / nv);
    }
    for (int g = 0; g < ni; g++) {
      for (size_t k = 0; k < Rn1.size(); k++) Rv.push_back(100.0 * (1.0 + 0.01 * g + 0.001 * (double)(k % 7)));
      for (size_t k = 0; k < Cn1.size(); k++) { Cv.push_back(1e-9 * (1.0 + 0.02 * g)); Cvp.push_back(0.0); }
      for (size_t k = 0; k < Ln1.size(); k++) { Lv.push_back(1e-6 * (1.0 + 0.03 * g)); Lip.push_back(0.0); }
      for (size_t k = 0; k < Dp.size(); k++) { Dis.push_back(1e-14 * (1.0 + 0.1 * g)); Dn.push_back(1.0 + 0.05 * (double)(k % 3)); Dvd.push_back(0.0); }
    }
    d.abi_version = SPICEY_ABI_VERSION; d.n_nodes = n + nv - 1; d.n_inst = ni;
    d.nR = (int32_t)Rn1.size(); d.nC = (int32_t)Cn1.size(); d.nL = (int32_t)Ln1.size(); d.nV = nv; d.nS = 0; d.nD = (int32_t)Dp.size();
    d.R_n1 = Rn1.data(); d.R_n2 = Rn2.data(); d.R_val = Rv.data();
    d.C_n1 = Cn1.data(); d.C_n2 = Cn2.data(); d.C_val = Cv.data(); d.C_vprev = Cvp.data();
    d.L_n1 = Ln1.data(); d.L_n2 = Ln2.data(); d.L_val = Lv.data(); d.L_iprev = Lip.data();
    d.V_n1 = Vn1.data(); d.V_n2 = Vn2.data();
    d.D_np = Dp.data(); d.D_nm = Dm.data(); d.D_is = Dis.data(); d.D_n = Dn.data(); d.D_vdprev = Dvd.data();
    d.n_out = 0; d.out_nodes = nullptr;
  }
};

int fail(const char *what) { fprintf(stderr, "ready_asan: %s\n", what); return 1; }

struct Out {
  std::vector<double> v, i, Cv, Li, Dv, zpar, src;
  std::vector<int32_t> it;
  std::vector<uint32_t> table;
  int64_t info[8] = {};
  int32_t rc = 0;
};

// own_src: every instance has a source table of its own (src_stride != 0); currents: 0 = a null current pointer
Out run(const Chain &ch, int ready, int64_t steps, int flags, bool own_src, bool currents) {
  Out o;
  const int T = 512;
  const int nCur = ch.d.nR + ch.d.nC + ch.d.nL + ch.d.nV + ch.d.nD;
  const size_t one = (size_t)(steps + 1) * ch.nv;
  o.src.resize(own_src ? one * ch.ni : one);
  for (size_t s = 0; s < o.src.size(); s++) o.src[s] = (((s / ch.nv) % (size_t)(steps + 1)) & 2 ? 3.0 : -3.0) * (1.0 + 0.1 * (double)(s % ch.nv) + 0.05 * (double)(s / one));
  o.zpar.assign((size_t)ch.ni * 2 * T * 5, 0.0);
  o.v.assign((size_t)ch.ni * (steps + 1) * ch.d.n_nodes, 0.0);
  if (currents) o.i.assign((size_t)ch.ni * (steps + 1) * nCur, 0.0);
  o.it.assign((size_t)ch.ni * (steps + 1), 0);
  o.table.assign((size_t)ch.ni * 64, 0u);
  o.Cv = ch.Cvp; o.Li = ch.Lip; o.Dv = ch.Dvd;
  o.rc = spicey_rahost_run(&ch.d, ready, T, steps, 1e-6, o.src.data(), own_src ? (int64_t)one : 0, o.zpar.data(), o.v.data(), currents ? o.i.data() : nullptr,
                           o.it.data(), o.Cv.data(), o.Li.empty() ? nullptr : o.Li.data(), o.Dv.data(), nullptr, flags, o.table.data(), o.info);
  return o;
}

bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

uint64_t word64(const Out &o, int g, int w, int run_words) {
  const uint32_t *t = o.table.data() + (size_t)g * run_words;
  return (uint64_t)t[w] | ((uint64_t)t[w + 1] << 32);
}

int one(const char *name, int n, int ni, int nv, bool ind, int64_t steps, bool own_src, bool currents) {
  Chain ch(n, ni, nv, ind);
  const Out off = run(ch, 0, steps, 0, own_src, currents), on = run(ch, 1, steps, 2, own_src, currents), rev = run(ch, 1, steps, 3, own_src, currents);
  printf("%s(%d) x %d, %d sources, %lld steps: rc %d %d %d, top of %lld rows\n", name, n, ni, nv, (long long)steps, off.rc, on.rc, rev.rc, (long long)on.info[2]);
  if (off.rc || on.rc || rev.rc) return fail("a run failed");
  for (const Out *o : {&on, &rev})
    if (!same(off.v, o->v) || !same(off.i, o->i) || off.it != o->it || !same(off.Cv, o->Cv) || !same(off.Li, o->Li) || !same(off.Dv, o->Dv)) return fail("ready arguments on and off differ");
  for (int32_t c : on.it)
    if (c < 1) return fail("an iteration count was not written");
  int32_t w[8];
  spicey_rahost_words(w);
  const int g = ni - 1;  // the last instance: its bases are the farthest into the buffers
  const size_t one_src = (size_t)(steps + 1) * nv;
  if (word64(on, g, w[0], w[7]) != (uint64_t)(uintptr_t)(on.zpar.data() + (size_t)g * (size_t)on.info[5])) return fail("record base");
  if (word64(on, g, w[1], w[7]) != (uint64_t)(uintptr_t)(on.src.data() + (own_src ? (size_t)g * one_src : 0))) return fail("source base");
  if (word64(on, g, w[2], w[7]) != (uint64_t)(uintptr_t)(on.it.data() + (size_t)g * (size_t)(steps + 1))) return fail("iteration-count base");
  if (word64(on, g, w[4], w[7]) != (currents ? (uint64_t)(uintptr_t)(on.i.data() + (size_t)g * (size_t)(steps + 1) * (size_t)on.info[7]) : 0u)) return fail("current row base");
  if (word64(off, g, w[0], w[7]) != (uint64_t)(uintptr_t)off.zpar.data()) return fail("the build without ready arguments moved the record pointer");
  double sum = 0.0;
  for (double v : on.v) sum += v;
  for (double v : on.i) sum += v;
  if (!(sum == sum)) return fail("NaN in the result");
  return 0;
}

int plan_of(bool knob, int64_t steps, bool want) {
  if (knob) setenv("SPICEY_NO_READY_ARGS", "1", 1);
  else unsetenv("SPICEY_NO_READY_ARGS");
  Chain ch(1000, 3, 1, false);
  SpiceyOptions opt{};
  opt.geometry = 2; opt.want_currents = 1;
  int64_t p[8];
  if (spicey_rahost_plan(&ch.d, &opt, 256, steps, p) != SPICEY_OK) return fail("plan");
  printf("plan, knob %d, %lld steps: ready %lld slots %lld early %lld fresh %lld packed %lld threads %lld lds %lld -> ready kernel %lld\n", (int)knob, (long long)steps,
         (long long)p[0], (long long)p[1], (long long)p[2], (long long)p[3], (long long)p[4], (long long)p[5], (long long)p[6], (long long)p[7]);
  unsetenv("SPICEY_NO_READY_ARGS");
  if (!p[1] || !p[2] || !p[3] || !p[4]) return fail("the plan did not take the packed fresh operand-slot build");
  if ((p[0] != 0) == knob) return fail("the knob and the plan's decision disagree");
  if ((p[7] != 0) != want) return fail("the launch's decision");
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad |= plan_of(false, 10000, true);
  bad |= plan_of(true, 10000, false);
  bad |= plan_of(false, 0xFFFFFFFEll, true);    // step + 1 still fits 32 bits
  bad |= plan_of(false, 0xFFFFFFFFll, false);   // ... no longer: the operand-slot kernel without ready arguments
  bad |= one("chain", 100, 3, 1, false, 6, false, true);     // one table for all instances
  bad |= one("chain", 100, 3, 1, false, 6, true, true);      // a table per instance: src_stride != 0
  bad |= one("chain", 1023, 1, 1, false, 3, false, true);    // every resident item exists
  bad |= one("sources", 200, 2, 3, false, 6, true, true);    // nV = 3: source base plus lane
  bad |= one("inductors", 200, 2, 1, true, 6, false, true);  // the inductor loop: its base and L_iprev from the complete structs
  bad |= one("chain", 100, 2, 1, false, 5, false, false);    // no currents: a null pointer stays null
  bad |= one("chain", 100, 2, 1, false, 0, true, true);      // no step beyond the first: nothing past the end of the source table
  printf(bad ? "ready_asan: FAILED\n" : "ready_asan: ok\n");
  return bad;
}
