// tests/addr_host/addr_asan.cpp — a stand-alone program (TEST INFRASTRUCTURE ONLY) for the address and undefined-behaviour
// sanitizers, linked with harness.cpp: the plan of a handle as spicey_create makes it, the prologue's re-encoding of B's
// descriptor fields as indices from the start of the workspace (TranPhases2::dd_addr / rhs_addr), and 8 steps of the emulated
// packed kernel reading and writing through those fields and through the record halves.  The workspace of every workgroup
// is a heap block of exactly spicey_lds_bytes bytes and every result, record and source buffer a heap block of exactly the
// planned size, so an index that is one base off lands in a red zone.  Every circuit runs with and without operand
// addresses and must give the same bytes.  Built and run by `make asan`; no GPU and no python involved.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spicey_hip.h"

extern "C" int32_t spicey_oahost_run(const SpiceyDesc *d, int32_t addr, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *zpar,
                                     double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags,
                                     uint32_t *regs_out, uint32_t *raw, int64_t *info16);
extern "C" int32_t spicey_oahost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out12);

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

int fail(const char *what) { fprintf(stderr, "addr_asan: %s\n", what); return 1; }

const int T = 512;

struct Out {
  std::vector<double> v, i, Cv, Dv, zpar, src;
  std::vector<int32_t> it;
  std::vector<uint32_t> regs, raw;
  int64_t info[16] = {};
  int32_t rc = 0;
};

Out run(const Chain &ch, int addr, int64_t steps, int flags) {
  Out o;
  const int nCur = ch.d.nR + ch.d.nC + ch.d.nV + ch.d.nD;
  o.src.resize((size_t)(steps + 1));
  for (size_t s = 0; s < o.src.size(); s++) o.src[s] = (s & 2) ? 3.0 : -3.0;
  o.zpar.assign((size_t)ch.ni * 2 * T * 5, 0.0);
  o.v.assign((size_t)ch.ni * (steps + 1) * ch.d.n_nodes, 0.0);
  o.i.assign((size_t)ch.ni * (steps + 1) * nCur, 0.0);
  o.it.assign((size_t)ch.ni * (steps + 1), 0);
  o.regs.assign((size_t)ch.ni * T * 14, 0u);
  o.raw.assign((size_t)T * 6, 0u);
  o.Cv = ch.Cvp; o.Dv = ch.Dvd;
  o.rc = spicey_oahost_run(&ch.d, addr, T, steps, 1e-6, o.src.data(), 0, o.zpar.data(), o.v.data(), o.i.data(), o.it.data(), o.Cv.data(), nullptr, o.Dv.data(), nullptr,
                           flags, o.regs.data(), o.raw.data(), o.info);
  return o;
}

bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

// the re-encoded field of a raw 15-bit dd field / 16-bit rhs field (index + 1 below the sign bit, 0: empty): index from W
uint32_t want_field(uint32_t f, uint32_t mask, uint32_t base, uint32_t minus0) { return f ? (f & mask) - 1u + base : minus0; }

int one(int n, int ni, int64_t steps) {
  Chain ch(n, ni);
  const Out off = run(ch, 0, steps, 0), on = run(ch, 1, steps, 2), rev = run(ch, 1, steps, 3);
  printf("chain(%d) x %d, %lld steps: rc %d %d %d, nW %lld nU %lld nGdyn %lld, largest index %lld, arena of %lld doubles\n", n, ni, (long long)steps, off.rc, on.rc, rev.rc,
         (long long)on.info[6], (long long)on.info[7], (long long)on.info[8], (long long)on.info[14], (long long)on.info[15]);
  if (off.rc || on.rc || rev.rc) return fail("a run failed");
  if (!on.info[5]) return fail("the program does not meet spicey_addr_fits");
  for (const Out *o : {&on, &rev})
    if (!same(off.v, o->v) || !same(off.i, o->i) || off.it != o->it || !same(off.Cv, o->Cv) || !same(off.Dv, o->Dv)) return fail("operand addresses on and off differ");
  // every field of the last instance's descriptors, against the program's own
  const uint32_t nW = (uint32_t)on.info[6], nU = (uint32_t)on.info[7], m0 = (uint32_t)on.info[9] + 1u;
  if (on.info[14] != (int64_t)m0 || (size_t)m0 >= (size_t)on.info[15]) return fail("the -0.0 slot is not the largest index, or lies outside the arena");
  const int g = ni - 1;
  for (int t = 0; t < T; t++) {
    const uint32_t *r = on.regs.data() + ((size_t)g * T + t) * 14, *w = on.raw.data() + (size_t)t * 6;
    for (int j = 0; j < 2; j++) {
      const bool mine = !(w[j] >> 31);
      const uint32_t f0 = mine ? w[j] & 0x7fffu : 0u, f1 = mine ? (w[j] >> 15) & 0x7fffu : 0u;
      if ((r[j] & 0x3fffu) != want_field(f0, 0x3fffu, nW + nU, m0) || ((r[j] >> 15) & 0x3fffu) != want_field(f1, 0x3fffu, nW + nU, m0)) return fail("a dd field");
      const bool row = w[3 + 2 * j] != 0xFFFFFFFFu;
      const uint32_t f[4] = {w[2 + 2 * j] & 0xffffu, w[2 + 2 * j] >> 16, w[3 + 2 * j] & 0xffffu, w[3 + 2 * j] >> 16};
      const uint32_t got[4] = {r[2 + 2 * j] & 0x3fffu, (r[2 + 2 * j] >> 16) & 0x3fffu, r[3 + 2 * j] & 0x3fffu, (r[3 + 2 * j] >> 16) & 0x3fffu};
      for (int q = 0; q < 4; q++)
        if (got[q] != want_field(row ? f[q] : 0u, 0x7fffu, nW, m0)) return fail("an rhs field");
    }
  }
  double sum = 0.0;
  for (double v : on.v) sum += v;
  for (double v : on.i) sum += v;
  if (!(sum == sum)) return fail("NaN in the result");
  return 0;
}

int plan_of(bool knob, int n, int ni) {
  if (knob) setenv("SPICEY_NO_OPERAND_ADDR", "1", 1);
  else unsetenv("SPICEY_NO_OPERAND_ADDR");
  Chain ch(n, ni);
  SpiceyOptions opt{};
  opt.geometry = 2; opt.want_currents = 1;
  int64_t p[12];
  const int32_t rc = spicey_oahost_plan(&ch.d, &opt, 256, 8, p);
  unsetenv("SPICEY_NO_OPERAND_ADDR");
  if (rc != SPICEY_OK) return fail("plan");
  printf("plan of chain(%d) x %d, knob %d: addr %lld ready %lld slots %lld early %lld fresh %lld packed %lld threads %lld lds %lld -> ready kernel %lld, with operand addresses %lld\n",
         n, ni, (int)knob, (long long)p[0], (long long)p[1], (long long)p[2], (long long)p[3], (long long)p[4], (long long)p[5], (long long)p[6], (long long)p[7], (long long)p[8],
         (long long)p[9]);
  if (!p[1] || !p[2] || !p[3] || !p[4] || !p[5] || !p[8]) return fail("the plan did not take the packed fresh ready-argument build");
  if ((p[0] != 0) == knob || (p[9] != 0) == knob || p[10] != p[0]) return fail("the knob and the plan's decision disagree");
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad |= plan_of(false, 100, 3);
  bad |= plan_of(true, 100, 3);
  bad |= plan_of(false, 1000, 2);
  bad |= plan_of(true, 1000, 2);
  bad |= one(100, 3, 8);    // most threads own no item: their descriptors name the -0.0 slot in every field
  bad |= one(1000, 2, 8);   // every resident item exists
  printf(bad ? "addr_asan: FAILED\n" : "addr_asan: ok\n");
  return bad;
}
