// tests/ac_exact_host/harness.cpp — the reference-order AC engine (spicey_amd/csrc/ac_exact_exec.h) on the CPU (TEST
// INFRASTRUCTURE).
//
// Runs the SAME plan (launch_plan.cpp, spicey_ac_exact_plan / spicey_ac_exact_chunk), the SAME stamp lists
// (ac_exact_plan.cpp) and the SAME phase code as the HIP kernel (ac_exact.hip), with `phase(f)` a loop over the thread ids
// (forwards or backwards, which exposes a dependence inside a phase) and the pivot search a serial scan.  Never loaded by
// spicey_amd/: libspicey_hip.so has no CPU path.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/ac_exact_exec.h"
#include "../../spicey_amd/csrc/ac_exact_plan.h"
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

int32_t plan_of(const SpiceyDesc *d, int32_t T, int32_t global, AcExactPlan &plan, HostAcExactProg &xp, std::string &err) {
  SpiceyOptions o{};
  o.interpreter = 3;
  o.threads = T;
  o.force_global = global;
  const int32_t rc = spicey_ac_exact_plan(d, o, plan, err);
  if (rc != SPICEY_OK) return rc;
  SpiceyDesc dd = *d;
  dd.nS = 0;
  dd.nD = 0;
  spicey_build_ac_exact(dd, plan.ws, xp);
  return rc;
}
}  // namespace

// The plan of an exact AC handle (threads 0 = automatic): info = {threads, lds (0/1), lds_bytes, n_var}; returns the
// status, the message in err.
extern "C" int32_t spicey_ac_exact_host_plan(const SpiceyDesc *d, int32_t T, int32_t global, int64_t slots, int64_t *info, char *err, int32_t cap) {
  AcExactPlan plan;
  HostAcExactProg xp;
  std::string msg;
  const int32_t rc = plan_of(d, T, global, plan, xp, msg);
  if (err && cap > 0) snprintf(err, (size_t)cap, "%s", msg.c_str());
  if (rc == SPICEY_OK) {
    info[0] = plan.T;
    info[1] = plan.lds ? 1 : 0;
    info[2] = (int64_t)plan.lds_bytes;
    info[3] = xp.hdr.n;
    info[4] = spicey_ac_exact_chunk(plan, slots);
    info[5] = plan.ws.cx * 16;
  }
  return rc;
}

// One sweep of every instance: out_v [n_inst][n_freq][n_out][2], out_i [n_inst][n_freq][n_cur][2] or null, status and
// skipped [n_inst * n_freq] per slot (0 / 1 / 5; nonzero multipliers the |f| < EPS test dropped).  global: the slots of a
// launch chunk share one slab (the GPU's global layout, stale between chunks), else a fresh buffer per slot (its LDS).
// Returns the status of the first failing slot (instance-major), its index in *first.
extern "C" int32_t spicey_ac_exact_host_run(const SpiceyDesc *d, int32_t T, int32_t global, int32_t reverse, int64_t n_freq, const double *freqs,
                                            const double *vph, double *out_v, double *out_i, int32_t *status, int64_t *skipped, int64_t *first) {
  AcExactPlan plan;
  HostAcExactProg xp;
  std::string err;
  int32_t rc = plan_of(d, T, global, plan, xp, err);
  if (rc != SPICEY_OK) { fprintf(stderr, "ac exact plan: %s\n", err.c_str()); return rc; }
  const SpiceyAcExactProg P = xp.bind(xp.blob.data());
  const int ni = d->n_inst;
  std::vector<double> rinv((size_t)ni * d->nR);
  for (size_t i = 0; i < rinv.size(); i++) rinv[i] = 1.0 / d->R_val[i];
  SpiceyAcExactRun R{};
  R.R_inv = rinv.data(); R.C_val = d->C_val; R.L_val = d->L_val;
  R.freqs = freqs; R.vph = vph; R.out_v = out_v; R.out_i = out_i; R.status = status; R.skipped = skipped;
  R.n_freq = n_freq; R.n_inst = ni;
  const int64_t slots = (int64_t)ni * n_freq, chunk = spicey_ac_exact_chunk(plan, slots);
  const size_t wsc = (size_t)P.ws_cx;
  const SpiceyCx nan2{NAN, NAN};
  std::vector<SpiceyCx> slab(global ? wsc * (size_t)chunk : 0, nan2), local;
  int32_t scal[4];
  for (int64_t s = 0; s < slots; s++) {
    SpiceyCx *ws;
    if (global) {
      ws = slab.data() + wsc * (size_t)(s % chunk);
    } else {
      local.assign(wsc, nan2);  // (what a kernel finds in LDS is undefined: no read before a write)
      ws = local.data();
    }
    for (int32_t &v : scal) v = -12345;
    SerialExec ex{plan.T, reverse != 0};
    spicey_ac_exact_solve(ex, P, R, ws, scal, s);
  }
  rc = SPICEY_OK;
  *first = -1;
  for (int64_t s = 0; s < slots; s++)
    if (status[s] != 0) {
      rc = status[s];
      *first = s;
      break;
    }
  return rc;
}

// The stamp lists: returns the number of entries; with room (cap_ent >= entries, cap_terms >= terms) also
// rc[e] = {row, column}, ptr[e + 1] = end of entry e's terms, terms[t] = {kind, elem, which, sub} (ac_exact_plan.h).
extern "C" int32_t spicey_ac_exact_host_lists(const SpiceyDesc *d, int32_t cap_ent, int32_t *rc, int32_t *ptr, int32_t cap_terms, int32_t *terms,
                                              int32_t *n_terms) {
  AcExactPlan plan;
  HostAcExactProg xp;
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

// V8's Math.hypot as the engine computes it (pairs [n][2] -> out [n])
extern "C" void spicey_ac_exact_host_hypot(int64_t n, const double *xy, double *out) {
  for (int64_t i = 0; i < n; i++) out[i] = spicey_v8_hypot(xy[2 * i], xy[2 * i + 1]);
}
