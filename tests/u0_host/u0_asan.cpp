// tests/u0_host/u0_asan.cpp — a stand-alone program (TEST INFRASTRUCTURE ONLY) for the address and undefined-behaviour
// sanitizers, linked with harness.cpp: the plan of a handle as spicey_create makes it, with and without
// SPICEY_NO_U0_RESIDENT, and 8 steps of the emulated packed kernel in the form that plan chooses — the prologue's load of
// level 0's row record into the registers and phase 0 running them, or the fetch under B.  The workspace of every workgroup
// is a heap block of exactly spicey_lds_bytes bytes and every result, record and source buffer a heap block of exactly the
// planned size.  Chains of 22 nodes (the smallest with a top: its level 0 is resident in the slots, so no plan takes the
// form) and of 1000 nodes (the benchmark's length: a row record in every thread); both plans must give the same bytes.
// Built and run by `make asan`; no GPU and no python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_u0host_run(const SpiceyDesc *d, int32_t resident, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *zpar,
                                     double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags,
                                     uint32_t *u0_out, uint32_t *raw, int64_t *info8, int32_t *err4, int64_t *solves_out);
extern "C" int32_t spicey_u0host_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out12);

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

int fail(const char *what) { fprintf(stderr, "u0_asan: %s\n", what); return 1; }

const int T = 512;

struct Out {
  std::vector<double> v, i, Cv, Dv, zpar, src;
  std::vector<int32_t> it;
  std::vector<uint32_t> u0, raw;
  int64_t info[8] = {};
  int64_t solves = 0;
  int32_t rc = 0;
};

Out run(const Chain &ch, int resident, int64_t steps, int flags) {
  Out o;
  const int nCur = ch.d.nR + ch.d.nC + ch.d.nV + ch.d.nD;
  o.src.resize((size_t)(steps + 1));
  for (size_t s = 0; s < o.src.size(); s++) o.src[s] = (s & 2) ? 3.0 : -3.0;
  o.zpar.assign((size_t)ch.ni * 2 * T * 5, 0.0);
  o.v.assign((size_t)ch.ni * (steps + 1) * ch.d.n_nodes, 0.0);
  o.i.assign((size_t)ch.ni * (steps + 1) * nCur, 0.0);
  o.it.assign((size_t)ch.ni * (steps + 1), 0);
  o.u0.assign((size_t)ch.ni * T * 8, 0u);
  o.raw.assign((size_t)T * 8, 0u);
  o.Cv = ch.Cvp; o.Dv = ch.Dvd;
  int32_t err4[4] = {0, 0, 0, 0};
  o.rc = spicey_u0host_run(&ch.d, resident, T, steps, 1e-6, o.src.data(), 0, o.zpar.data(), o.v.data(), o.i.data(), o.it.data(), o.Cv.data(), nullptr, o.Dv.data(), nullptr,
                           flags, o.u0.data(), o.raw.data(), o.info, err4, &o.solves);
  return o;
}

bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

// the form the plan of a handle takes, with the knob or without: 1 / 0, -1 on an error
int planned(const Chain &ch, bool knob, int64_t steps) {
  if (knob) setenv("SPICEY_NO_U0_RESIDENT", "1", 1);
  else unsetenv("SPICEY_NO_U0_RESIDENT");
  SpiceyOptions opt{};
  opt.geometry = 2; opt.want_currents = 1;
  int64_t p[12];
  const int32_t rc = spicey_u0host_plan(&ch.d, &opt, 256, steps, p);
  unsetenv("SPICEY_NO_U0_RESIDENT");
  if (rc != SPICEY_OK) return -1;
  printf("plan of chain(%d) x %d, knob %d: u0_resident %lld top_regs %lld addr %lld packed %lld fresh %lld threads %lld, level 0: rows %lld records %lld remainder %lld -> form %lld\n",
         ch.n, ch.ni, (int)knob, (long long)p[0], (long long)p[1], (long long)p[2], (long long)p[3], (long long)p[4], (long long)p[5], (long long)p[9], (long long)p[10],
         (long long)p[11], (long long)p[8]);
  if (!p[1] || !p[2] || !p[3] || !p[4] || !p[7]) return -1;  // (not the packed fresh register-exchange-top build)
  return (int)p[8];
}

// `takes`: whether the plan of such a handle takes the form without the knob (level 0 of a short chain is resident in the
// slots: nothing is streamed, and both plans run the same kernel)
int one(int n, int ni, int64_t steps, int takes) {
  Chain ch(n, ni);
  const int with_knob = planned(ch, true, steps), without = planned(ch, false, steps);
  if (with_knob != 0) return fail("the knob does not keep the fetching kernel");
  if (without != takes) return fail(takes ? "the plan does not take the resident record" : "the plan takes the resident record where level 0 is not streamed");
  const Out off = run(ch, with_knob, steps, 0), on = run(ch, without, steps, 2), rev = run(ch, without, steps, 3);
  printf("chain(%d) x %d, %lld steps: rc %d %d %d, %lld row records, %lld solves\n", n, ni, (long long)steps, off.rc, on.rc, rev.rc, (long long)on.info[1], (long long)on.solves);
  if (off.rc || on.rc || rev.rc) return fail("a run failed");
  for (const Out *o : {&on, &rev})
    if (!same(off.v, o->v) || !same(off.i, o->i) || off.it != o->it || !same(off.Cv, o->Cv) || !same(off.Dv, o->Dv) || off.solves != o->solves) return fail("the resident record on and off differ");
  // every thread of every instance holds the program's record, or zeros beyond the count
  if (takes)
  for (int g = 0; g < ni; g++)
    for (int t = 0; t < T; t++)
      if (memcmp(on.u0.data() + ((size_t)g * T + t) * 8, on.raw.data() + (size_t)t * 8, 32) != 0) return fail("a record word");
  for (int t = takes ? (int)on.info[1] : T; t < T; t++)
    for (int w = 0; w < 8; w++)
      if (on.u0[(size_t)t * 8 + w] != 0u) return fail("a thread beyond the record count does not hold zeros");
  double sum = 0.0;
  for (double v : on.v) sum += v;
  for (double v : on.i) sum += v;
  if (!(sum == sum)) return fail("NaN in the result");
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad |= one(22, 3, 8, 0);
  bad |= one(1000, 2, 8, 1);
  printf(bad ? "u0_asan: FAILED\n" : "u0_asan: ok\n");
  return bad;
}
