// tests/early_host/harness.cpp — CPU harness of the early-prefetch builds (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// build <4, 2, 2> in three forms: without the parameter record (SpiceyRun::zpar null — the loads of the plain build), with
// the record on the emulator's own executor (the fetch at the tail of the peeled last factor phase), and with the record on
// an executor that has `idle_waves` (the fetch in the phase of the tridiagonal top, as on the GPU).  On request the record,
// the workspace and every thread's prefetch registers start as NaN.  Also the launch plan's decision and the record's size.
#include "../emul/emul.cpp"

#include <cmath>
#include <limits>

namespace {

// The emulator's executor with the GPU executor's extra entry point.  The threads beside the first wave run `g` BEFORE
// the steps, the first wave after them: on the GPU the idle waves run it while the top is under way, and nothing it does
// may depend on which comes first.
struct SeqExecIdle : SeqExec {
  static constexpr bool idle_waves = true;
  template <class F, class G>
  void wave_lockstep_keep_then(int nlanes, int nsteps, F f, G g) {
    if (!reverse) for (int t = 64; t < T; t++) g(t);
    else for (int t = T - 1; t >= 64; t--) g(t);
    wave_lockstep_keep(nlanes, nsteps, f);
    const int n = T < 64 ? T : 64;
    if (!reverse) for (int t = 0; t < n; t++) g(t);
    else for (int t = n - 1; t >= 0; t--) g(t);
  }
};

typedef ResRegs<1, 4, 2, 2> FreshRegs;

template <bool EP, class Exec>
void run_one(Exec &ex, const SpiceyProg &P, const SpiceyResident &Q, const SpiceyRun &R, WgCtx<1> &c, int g, int T, bool nan_regs) {
  std::vector<FreshRegs> regs(T);
  if (nan_regs)
    for (FreshRegs &r : regs) {
      for (auto &item : r.pf) for (double &v : item) v = std::numeric_limits<double>::quiet_NaN();
      r.srcn = std::numeric_limits<double>::quiet_NaN();
    }
  ex.rr = &regs;
  spicey_tran_run_v2<1, 4, 2, 2, false, -1, EP>(ex, P, Q, R, c, g);
}

}  // namespace

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d`.  mode 0: no record; 1: record, the
// emulator's executor; 2: record, an executor with idle waves.  flags bit 0: threads of a phase in reverse order, bit 1:
// the workspace, the record and the prefetch registers start as NaN.  info6 = {nV, nS, pcr_n, fresh_fill, doubles of the
// record, doubles of it that the run left as NaN}.
extern "C" int32_t spicey_early_run(const SpiceyDesc *d, int32_t mode, int32_t T, int64_t steps, double dt, const double *src, double *out_v, double *out_i,
                                    int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags, int64_t *info6) {
  HostProgram hp;
  std::string err;
  int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return rc;
  if (hp.structurally_singular || !hp.hdr.has16 || !hp.hdr.fresh_fill || T <= 0 || (T & 63) || mode < 0 || mode > 2) return SPICEY_ERR_BAD_DESC;
  SpiceyProg P = hp.bind(hp.blob.data());
  const int ni = d->n_inst;
  SpiceyRun R{};
  R.n_inst = ni; R.want_currents = out_i != nullptr; R.steps = steps; R.dt = dt;
  R.R_val = d->R_val; R.C_val = d->C_val; R.L_val = d->L_val;
  R.S_ron = d->S_ron; R.S_roff = d->S_roff; R.S_von = d->S_von; R.S_voff = d->S_voff;
  R.D_is = d->D_is; R.D_n = d->D_n;
  R.C_vprev = C_vprev; R.L_iprev = L_iprev; R.D_vdprev = D_vdprev; R.S_ison = S_ison;
  std::vector<double> gstat((size_t)ni * P.nGstat), statv((size_t)ni * P.nLU), rcoef((size_t)ni * (P.nRhsIdx + 1)), dpar((size_t)ni * (P.nD + 1) * 2);
  R.gstat = gstat.data(); R.statv = statv.data(); R.rcoef = rcoef.data(); R.dpar = dpar.data();
  R.src = src; R.out_v = out_v; R.out_i = out_i; R.iters = iters;
  std::vector<int32_t> status((size_t)ni * 4);
  std::vector<unsigned long long> solves(ni);
  R.status = status.data(); R.solves = solves.data();
  const bool nan = (flags & 2) != 0;
  const double fill = nan ? std::numeric_limits<double>::quiet_NaN() : 0.0;
  // the record as the handle sizes it: five doubles per resident item, NEL = 2 items per thread
  std::vector<double> zpar(mode ? (size_t)ni * 2 * (size_t)T * 5 : 0, fill);
  R.zpar = mode ? zpar.data() : nullptr;
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  SpiceyResident Q = hr.bind(hr.blob.data());
  for (int g = 0; g < ni; g++) {
    std::vector<double> W((size_t)P.nW, fill), u((size_t)P.nU + 1, fill), gd((size_t)P.nGdyn + 1, fill);
    std::vector<int32_t> ison((size_t)P.nS + 1), fl(4);
    std::vector<uint32_t> tail((size_t)(hr.tail_n + 6) * 64 * 4);
    WgCtx<1> c;
    c.W = W.data(); c.u = u.data(); c.gd = gd.data(); c.ison = ison.data(); c.flags = fl.data(); c.tail = tail.data(); c.G = nullptr;
    c.valid[0] = true; c.inst[0] = g;
    if (mode == 2) {
      SeqExecIdle ex;
      ex.T = T; ex.reverse = (flags & 1) != 0;
      run_one<true>(ex, P, Q, R, c, g, T, nan);
    } else {
      SeqExec ex{T, (flags & 1) != 0};
      if (mode == 1) run_one<true>(ex, P, Q, R, c, g, T, nan);
      else run_one<false>(ex, P, Q, R, c, g, T, nan);
    }
  }
  if (info6) {
    int64_t left = 0;
    for (double v : zpar) left += std::isnan(v) ? 1 : 0;
    info6[0] = P.nV; info6[1] = P.nS; info6[2] = P.pcr_n; info6[3] = P.fresh_fill; info6[4] = (int64_t)zpar.size(); info6[5] = left;
  }
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there): out6 = {early, fresh, packed, threads,
// index of the v2 build it launches, doubles of the parameter record the handle will own}
extern "C" int32_t spicey_early_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t *out6) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  out6[0] = plan.early; out6[1] = plan.fresh; out6[2] = plan.packed; out6[3] = plan.T;
  out6[4] = plan.interp == 2 ? spicey_v2_shape(plan.T, plan.packed, hp.hdr.hybrid != 0, plan.packed && hp.hdr.fresh_fill != 0) : -1;
  out6[5] = (int64_t)spicey_zpar_doubles(plan, hp);
  return SPICEY_OK;
}
