// tests/ready_host/harness.cpp — CPU harness of the ready-argument builds (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// operand-slot build <4, 2, 2> with and without ready arguments (tran_v2_run.h: RA).  Every workgroup lives in ONE arena of
// exactly spicey_lds_bytes bytes, laid out as the kernel lays out its LDS; the record, the result arrays and the source
// table are the caller's buffers of exactly the planned sizes.  After each instance's run the run-wide block of its phase
// table is copied out, with the pointers and strides that its rebased words are made of.  Also the launch plan's decision.
#include "../emul/emul.cpp"

#include <cmath>
#include <cstring>
#include <limits>

namespace {

// the emulator's executor with the GPU executor's entry point for the phase of the tridiagonal top (tests/early_host)
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

// the LDS arena of one workgroup (K = 1, LDS workspace), as spicey_tran_kernel_v2 lays it out
struct Arena {
  std::vector<double> mem;  // (doubles: 8-byte alignment for every section)
  WgCtx<1> c;
  Arena(const SpiceyProg &P, int tail_n, double fill, int inst) {
    const size_t bytes = spicey_lds_bytes(P, 1, true, tail_n);
    mem.assign(bytes / sizeof(double), fill);
    char *base = (char *)mem.data();
    c.W = mem.data();
    c.G = nullptr;
    c.u = c.W + P.nW;
    c.gd = c.u + P.nU;
    c.ison = (int32_t *)(c.gd + P.nGdyn);
    c.flags = c.ison + P.nS;
    for (int i = 0; i < P.nS + 4; i++) c.ison[i] = 0;
    const size_t off_prof = (((size_t)P.nW + P.nU + P.nGdyn) * sizeof(double) + ((size_t)P.nS + 4) * sizeof(int32_t) + 15) & ~(size_t)15;
    c.tail = (uint32_t *)(base + off_prof + SPICEY_PH_SLOTS * sizeof(unsigned long long));
    c.valid[0] = true; c.inst[0] = inst;
  }
};

}  // namespace

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d` on the operand-slot build with idle
// waves; ready: 1 = its ready-argument form.  src: the source table, instance g's at src + g x src_stride (0: one for all).
// zpar: ni x 2 x T x 5 doubles (the caller's: exactly spicey_zpar_doubles of such a plan).  flags bit 0: threads of a phase
// in reverse order, bit 1: the arena and the prefetch registers start as NaN.  table: ni x SPICEY_PT_RUN words, the
// run-wide block of each instance's phase table after its run.  info8 = {nV, nS, pcr_n, fresh_fill, spicey_slots_fit,
// 2 x T x 5 (doubles of one instance's record), nOut, nCur}.
extern "C" int32_t spicey_rahost_run(const SpiceyDesc *d, int32_t ready, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *zpar,
                                     double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags,
                                     uint32_t *table, int64_t *info8) {
  HostProgram hp;
  std::string err;
  int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return rc;
  if (hp.structurally_singular || !hp.hdr.has16 || !hp.hdr.fresh_fill || T <= 0 || (T & 63)) return SPICEY_ERR_BAD_DESC;
  if (ready && !spicey_ready_steps_ok(steps)) return SPICEY_ERR_BAD_DESC;  // (the launch would not have chosen the build)
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
  R.src = src; R.src_stride = src_stride; R.out_v = out_v; R.out_i = out_i; R.iters = iters;
  std::vector<int32_t> status((size_t)ni * 4);
  std::vector<unsigned long long> solves(ni);
  R.status = status.data(); R.solves = solves.data();
  R.zpar = zpar;
  const bool nan = (flags & 2) != 0;
  const double fill = nan ? std::numeric_limits<double>::quiet_NaN() : 0.0;
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  SpiceyResident Q = hr.bind(hr.blob.data());
  const bool fit = spicey_slots_fit(P, hr.tail_n);
  if (!fit || !spicey_pt_runtime_choice(P, Q)) return SPICEY_ERR_BAD_DESC;  // (the plan would not have chosen either build)
  for (int g = 0; g < ni; g++) {
    Arena a(P, hr.tail_n, fill, g);
    std::vector<FreshRegs> regs(T);
    if (nan)
      for (FreshRegs &r : regs) {
        for (auto &item : r.pf) for (double &v : item) v = std::numeric_limits<double>::quiet_NaN();
        r.srcn = std::numeric_limits<double>::quiet_NaN();
      }
    SeqExecIdle ex;
    ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
    if (ready) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true>(ex, P, Q, R, a.c, g);
    else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, false>(ex, P, Q, R, a.c, g);
    if (table) memcpy(table + (size_t)g * SPICEY_PT_RUN, a.c.tail + spicey_pt_base_words(P.pcr_n), SPICEY_PT_RUN * sizeof(uint32_t));
  }
  if (info8) {
    info8[0] = P.nV; info8[1] = P.nS; info8[2] = P.pcr_n; info8[3] = P.fresh_fill; info8[4] = fit; info8[5] = 2 * (int64_t)T * 5;
    info8[6] = P.nOut; info8[7] = P.nCur;
  }
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}

// The index of a table word by name: out = {ZPAR, SRC, ITERS, OUT_V, OUT_I, C_VPREV, D_VDPREV, RUN}
extern "C" void spicey_rahost_words(int32_t *out8) {
  out8[0] = SPICEY_PT_ZPAR; out8[1] = SPICEY_PT_SRC; out8[2] = SPICEY_PT_ITERS; out8[3] = SPICEY_PT_OUT_V; out8[4] = SPICEY_PT_OUT_I;
  out8[5] = SPICEY_PT_C_VPREV; out8[6] = SPICEY_PT_D_VDPREV; out8[7] = SPICEY_PT_RUN;
}

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there), and what a run of `steps` steps on
// such a handle launches: out8 = {ready, slots, early, fresh, packed, threads, lds_bytes, spicey_ready_run(plan, steps)}
extern "C" int32_t spicey_rahost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out8) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  out8[0] = plan.ready; out8[1] = plan.slots; out8[2] = plan.early; out8[3] = plan.fresh; out8[4] = plan.packed; out8[5] = plan.T;
  out8[6] = (int64_t)plan.lds_bytes; out8[7] = spicey_ready_run(plan, steps);
  return SPICEY_OK;
}
