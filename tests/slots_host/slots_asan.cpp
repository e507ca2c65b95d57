// tests/slots_host/slots_asan.cpp — a stand-alone program (TEST INFRASTRUCTURE ONLY) for the address and undefined-behaviour
// sanitizers, linked with harness.cpp: slot placement (tran_pt_layout.h), the launch plan's decision (launch_plan.cpp), the
// re-encoding of the resident terminal indices and of phase B's descriptors, and the emulator's B and Z reading through
// them, in an arena of exactly spicey_lds_bytes per workgroup (heap: the sanitizer guards both ends, and the slots are its
// last sixteen bytes).  Every circuit runs with and without the slots and must give the same bytes.  Built and run by
// `make asan`; no GPU and no python involved.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_slots_run(const SpiceyDesc *d, int32_t slots, int32_t T, int64_t steps, double dt, const double *src, double *out_v, double *out_i,
                                    int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags, int64_t *info8);
extern "C" void spicey_slots_where(int32_t nW, int32_t nU, int32_t nGdyn, int32_t nS, int32_t pcr_n, int32_t pcr_level, int32_t tail_n, int64_t *out4);
extern "C" int32_t spicey_slots_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t *out6);

namespace {

// V1 n1 0, then per stage k: R n_k n_k+1, C and D between n_k+1 and ground — `reversed`: ground first (and the diode points
// the other way); `dense`: every fourth stage an antiparallel diode pair and a capacitor across the resistor, every eighth a
// third diode to ground (rows of four and five contributions, entries of two and three conductances); `zz`: one resistor
// and one capacitor between ground and ground
struct Chain {
  int n, ni;
  std::vector<int32_t> Rn1, Rn2, Cn1, Cn2, Vn1, Vn2, Dp, Dm;
  std::vector<double> Rv, Cv, Cvp, Dis, Dn, Dvd;
  SpiceyDesc d{};
  Chain(int n_, int ni_, bool reversed, bool dense, bool zz) : n(n_), ni(ni_) {
    for (int k = 1; k < n; k++) {
      Rn1.push_back(k); Rn2.push_back(k + 1);
      Cn1.push_back(reversed ? 0 : k + 1); Cn2.push_back(reversed ? k + 1 : 0);
      Dp.push_back(reversed ? 0 : k + 1); Dm.push_back(reversed ? k + 1 : 0);
      if (dense && k % 4 == 0) {
        Dp.push_back(k); Dm.push_back(k + 1);
        Dp.push_back(k + 1); Dm.push_back(k);
        Cn1.push_back(k); Cn2.push_back(k + 1);
      }
      if (dense && k % 8 == 0) { Dp.push_back(k + 1); Dm.push_back(0); }
    }
    if (zz) { Rn1.push_back(0); Rn2.push_back(0); Cn1.push_back(0); Cn2.push_back(0); }
    Vn1 = {1}; Vn2 = {0};
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

int fail(const char *what) { fprintf(stderr, "slots_asan: %s\n", what); return 1; }

struct Out {
  std::vector<double> v, i, Cv, Dv;
  std::vector<int32_t> it;
  int64_t info[8] = {};
  int32_t rc = 0;
};

Out run(const Chain &ch, int slots, int64_t steps, int flags) {
  Out o;
  const int nCur = ch.d.nR + ch.d.nC + ch.d.nV + ch.d.nD;
  std::vector<double> src((size_t)(steps + 1));
  for (int64_t s = 0; s <= steps; s++) src[(size_t)s] = (s & 2) ? 3.0 : -3.0;  // both polarities: reversed diodes conduct too
  o.v.assign((size_t)ch.ni * (steps + 1) * ch.d.n_nodes, 0.0);
  o.i.assign((size_t)ch.ni * (steps + 1) * nCur, 0.0);
  o.it.assign((size_t)ch.ni * (steps + 1), 0);
  o.Cv = ch.Cvp; o.Dv = ch.Dvd;
  o.rc = spicey_slots_run(&ch.d, slots, 512, steps, 1e-6, src.data(), o.v.data(), o.i.data(), o.it.data(), o.Cv.data(), nullptr, o.Dv.data(), nullptr, flags, o.info);
  return o;
}

bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

int one(const char *name, int n, int ni, bool reversed, bool dense, bool zz, int64_t steps) {
  Chain ch(n, ni, reversed, dense, zz);
  const Out off = run(ch, 0, steps, 0), on = run(ch, 1, steps, 2), rev = run(ch, 1, steps, 3);  // (on: NaN arena; rev: and threads in reverse)
  printf("%s(%d) x %d, %lld steps: rc %d %d %d, slots fit %lld at index %lld, top of %lld rows\n", name, n, ni, (long long)steps, off.rc, on.rc, rev.rc,
         (long long)on.info[4], (long long)on.info[5], (long long)on.info[2]);
  if (off.rc || on.rc || rev.rc) return fail("a run failed");
  if (!on.info[4]) return fail("the slots did not fit");
  for (const Out *o : {&on, &rev}) {
    if (!same(off.v, o->v) || !same(off.i, o->i) || off.it != o->it || !same(off.Cv, o->Cv) || !same(off.Dv, o->Dv)) return fail("slots on and off differ");
    if (o->info[6] != 0 || (uint64_t)o->info[7] != 0x8000000000000000ull) return fail("a slot lost its constant");
  }
  double sum = 0.0;
  for (double v : on.v) sum += v;
  for (double v : on.i) sum += v;
  if (!(sum == sum)) return fail("NaN in the result");
  return 0;
}

int placement() {
  int64_t w[4];
  for (int nS = 0; nS < 6; nS++)
    for (int nG = 0; nG < 3; nG++) {
      spicey_slots_where(701, 33, 7 + nG, nS, 17, 2, 0, w);
      if (!w[0] || w[2] != w[3]) return fail("the slots are not the last sixteen bytes of the arena");
    }
  spicey_slots_where(7000, 3001, 999, 0, 64, 5, 0, w);
  if (w[0]) return fail("slots placed over the phase table's last row");
  spicey_slots_where(60000, 4000, 1000, 0, 40, 3, 0, w);
  if (w[0]) return fail("slots placed beyond the reach of a 16-bit index");
  spicey_slots_where(7000, 12000, 3700, 0, 40, 3, 0, w);
  if (w[0]) return fail("slots placed beyond the reach of a 14-bit descriptor field");
  return 0;
}

int plan_of(bool knob) {
  if (knob) setenv("SPICEY_NO_OPERAND_SLOTS", "1", 1);
  else unsetenv("SPICEY_NO_OPERAND_SLOTS");
  Chain ch(1000, 3, false, false, false);
  SpiceyOptions opt{};
  opt.geometry = 2; opt.want_currents = 1;
  int64_t p[6];
  if (spicey_slots_plan(&ch.d, &opt, 256, p) != SPICEY_OK) return fail("plan");
  printf("plan, knob %d: slots %lld early %lld fresh %lld packed %lld threads %lld lds %lld\n", (int)knob, (long long)p[0], (long long)p[1], (long long)p[2],
         (long long)p[3], (long long)p[4], (long long)p[5]);
  if (!p[1] || !p[2] || !p[3]) return fail("the plan did not take the packed fresh early-prefetch build");
  if ((p[0] != 0) == knob) return fail("the knob and the plan's decision disagree");
  unsetenv("SPICEY_NO_OPERAND_SLOTS");
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad |= placement();
  bad |= plan_of(false);
  bad |= plan_of(true);
  bad |= one("chain", 100, 2, false, false, false, 6);      // most threads own nothing: every index names a slot
  bad |= one("chain", 1023, 1, false, false, false, 3);     // every resident item exists
  bad |= one("reversed", 200, 2, true, false, true, 6);     // ground first, and elements between two grounds
  bad |= one("dense", 200, 1, false, true, false, 6);       // four contributions, two conductances, the list forms
  printf(bad ? "slots_asan: FAILED\n" : "slots_asan: ok\n");
  return bad;
}
