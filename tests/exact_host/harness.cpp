// tests/exact_host/harness.cpp — the reference-order engine (spicey_amd/csrc/exact_exec.h) on the CPU (TEST INFRASTRUCTURE).
//
// Runs the SAME plan (launch_plan.cpp, interpreter 3), the SAME stamp lists (exact_plan.cpp) and the SAME phase code as the
// HIP kernel (exact.hip), with `phase(f)` a loop over the thread ids (forwards or backwards, which exposes a dependence
// inside a phase) and the pivot search a serial scan.  Never loaded by spicey_amd/: libspicey_hip.so has no CPU path.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/exact_exec.h"
#include "../../spicey_amd/csrc/exact_plan.h"
#include "../../spicey_amd/csrc/launch_plan.h"

namespace {
struct SerialExec {
  int T;
  bool reverse;
  int threads() const { return T; }
  int atomic_add(int32_t *p, int v) { const int o = *p; *p += v; return o; }
  template <class F>
  void phase(int, F f) {
    if (!reverse)
      for (int t = 0; t < T; t++) f(t);
    else
      for (int t = T - 1; t >= 0; t--) f(t);
  }
  template <class G>
  void argmax(int count, G get, double &bv, int &bi) {
    bv = -1.0;
    bi = INT_MAX;
    for (int j = 0; j < count; j++) {
      const double v = get(j);
      if (v > bv) { bv = v; bi = j; }
    }
  }
};

int32_t plan_of(const SpiceyDesc *d, int32_t T, int32_t global, LaunchPlan &plan, HostExactProg &xp, std::string &err) {
  SpiceyOptions o{};
  o.interpreter = 3;
  o.threads = T;
  o.force_global = global;
  const PlanDevice dev{[](int, int *n, std::string &) { *n = 256; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, err);
  if (rc == SPICEY_OK) spicey_build_exact(*d, plan.xws, xp);
  return rc;
}
}  // namespace

// One run of every instance.  State arrays [n_inst][n<kind>] in / out; skip [n_inst] (nonzero multipliers the |f| < EPS
// test dropped); lin_err [n_inst][steps + 1] or null; err4 = {code, inst, step, iter} of the first failing instance;
// info (optional) = the plan.  global: the workspace of every instance in one slab (the GPU's global layout), else a
// fresh buffer per instance (its LDS).
extern "C" int32_t spicey_exact_host_run(const SpiceyDesc *d, int32_t T, int32_t global, int32_t reverse, int64_t steps, double dt, const double *src,
                                         double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison,
                                         int64_t *skip, double *lin_err, int32_t *err4, SpiceyInfo *info) {
  LaunchPlan plan;
  HostExactProg xp;
  std::string err;
  int32_t rc = plan_of(d, T, global, plan, xp, err);
  if (rc != SPICEY_OK) { fprintf(stderr, "exact plan: %s\n", err.c_str()); return rc; }
  if (info) {
    HostProgram hp;
    hp.hdr.n = xp.hdr.n; hp.hdr.nOut = xp.hdr.nOut; hp.hdr.nCur = xp.hdr.nCur;
    fill_info(plan, hp, HostResident(), SpiceyOptions{}, info);
  }
  const SpiceyExactProg P = xp.bind(xp.blob.data());
  const int ni = d->n_inst;
  std::vector<int32_t> status((size_t)ni * 4, -1);
  std::vector<unsigned long long> solves((size_t)ni), skipc((size_t)ni);
  SpiceyRun R{};
  R.n_inst = ni;
  R.steps = steps;
  R.dt = dt;
  R.R_val = d->R_val; R.C_val = d->C_val; R.L_val = d->L_val;
  R.S_ron = d->S_ron; R.S_roff = d->S_roff; R.S_von = d->S_von; R.S_voff = d->S_voff;
  R.D_is = d->D_is; R.D_n = d->D_n;
  R.C_vprev = C_vprev; R.L_iprev = L_iprev; R.D_vdprev = D_vdprev; R.S_ison = S_ison;
  R.src = src; R.out_v = out_v; R.out_i = out_i; R.iters = iters;
  R.status = status.data(); R.solves = solves.data(); R.skip_risk = skipc.data();
  R.lin_err = reinterpret_cast<unsigned long long *>(lin_err);
  const size_t wsd = (size_t)P.ws_doubles;
  std::vector<double> slab(global ? wsd * ni : 0, NAN), local;
  int32_t scal[8];
  for (int inst = 0; inst < ni; inst++) {
    double *ws;
    if (global) {
      ws = slab.data() + wsd * inst;
    } else {
      local.assign(wsd, NAN);  // (what a kernel finds in LDS is undefined: no read before a write)
      ws = local.data();
    }
    for (int32_t &s : scal) s = -12345;
    SerialExec ex{plan.T, reverse != 0};
    spicey_exact_run(ex, P, R, ws, scal, inst, inst);
  }
  rc = SPICEY_OK;
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4] != 0 && (rc == SPICEY_OK || status[(size_t)g * 4 + 2] < err4[2])) {
      rc = status[(size_t)g * 4];
      for (int k = 0; k < 4; k++) err4[k] = status[(size_t)g * 4 + k];
    }
  for (int i = 0; i < ni; i++) skip[i] = (int64_t)skipc[i];
  return rc;
}

// The stamp lists: returns the number of entries; with room (cap_ent >= entries, cap_terms >= terms) also
// rc[e] = {row, column}, ptr[e + 1] = end of entry e's terms, terms[t] = {kind, elem, which, sub} (exact_plan.h).
extern "C" int32_t spicey_exact_host_lists(const SpiceyDesc *d, int32_t cap_ent, int32_t *rc, int32_t *ptr, int32_t cap_terms, int32_t *terms,
                                           int32_t *n_terms) {
  LaunchPlan plan;
  HostExactProg xp;
  std::string err;
  if (plan_of(d, 0, 0, plan, xp, err) != SPICEY_OK) return -1;
  const int ne = xp.hdr.nEnt;
  *n_terms = (int32_t)xp.ent_src.size();
  if (cap_ent < ne || cap_terms < *n_terms) return ne;
  ptr[0] = 0;
  for (int e = 0; e < ne; e++) {
    rc[2 * e] = (int32_t)(xp.ent_pos[e] / (uint32_t)xp.hdr.ld);
    rc[2 * e + 1] = (int32_t)(xp.ent_pos[e] % (uint32_t)xp.hdr.ld);
    ptr[e + 1] = (int32_t)xp.ent_ptr[e + 1];
  }
  for (size_t t = 0; t < xp.ent_src.size(); t++) {
    const SpiceyExactTerm m = xp.decode(xp.ent_src[t]);
    terms[4 * t] = m.kind; terms[4 * t + 1] = m.elem; terms[4 * t + 2] = m.which; terms[4 * t + 3] = m.sub;
  }
  return ne;
}
