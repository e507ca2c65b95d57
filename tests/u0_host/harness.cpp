// tests/u0_host/harness.cpp — CPU harness of the resident level-0 record (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// operand-address build <4, 2, 2> with the register-exchange-top flag, with and without the resident level-0 record
// (tran_v2_run.h: UR).  Every workgroup lives in ONE arena of exactly spicey_lds_bytes bytes, laid out as the kernel lays
// out its LDS (tests/addr_host).  After each instance's run the eight record words of every thread are copied out, next
// to the program's own record of that thread.  Also the launch plan's decision, and the port of the device library's
// exp (tran_common.h: spicey_exp_port) as the host compiles it.
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

// the LDS arena of one workgroup (K = 1, LDS workspace), as spicey_tran_kernel_v2 lays it out: a heap block of exactly
// spicey_lds_bytes bytes
struct Arena {
  size_t n;
  double *mem;  // (doubles: 8-byte alignment for every section)
  WgCtx<1> c;
  Arena(const SpiceyProg &P, int tail_n, double fill, int inst) {
    const size_t bytes = spicey_lds_bytes(P, 1, true, tail_n);
    n = bytes / sizeof(double);
    mem = new double[n];
    for (size_t i = 0; i < n; i++) mem[i] = fill;
    char *base = (char *)mem;
    c.W = mem;
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
  ~Arena() { delete[] mem; }
  Arena(const Arena &) = delete;
  Arena &operator=(const Arena &) = delete;
};

}  // namespace

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d` on the operand-address build with idle
// waves; resident: 1 = the form with the resident level-0 record — refused (SPICEY_ERR_BAD_DESC) where
// spicey_u0_resident_fits does not hold, as the plan would refuse it.  src: the source table, instance g's at
// src + g x src_stride (0: one for all).  zpar: ni x 2 x T x 5 doubles.  flags bit 0: threads of a phase in reverse order,
// bit 1: the arena, the prefetch registers and the record words start as NaN / all ones.
// u0: ni x T x 8 words, ResRegs::u0 of every thread after the run.  raw: T x 8 words, the program's row record `tid` of
// factor phase 0 (zeros for a thread at or beyond the record count, or where the phase is not streamed as row records).
// err4: the status words {code, inst, step, iter} of the first workgroup that failed.
// info8 = {st_desc[0] (row-record encoding), st_desc[2] (row records), st_desc[5] (generic remainder), spicey_u0_resident_fits,
// pcr_n, pcr_level, nLevels, spicey_addr_fits}.
extern "C" int32_t spicey_u0host_run(const SpiceyDesc *d, int32_t resident, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *zpar,
                                     double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags,
                                     uint32_t *u0_out, uint32_t *raw, int64_t *info8, int32_t *err4, int64_t *solves_out) {
  HostProgram hp;
  std::string err;
  int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return rc;
  if (hp.structurally_singular || !hp.hdr.has16 || !hp.hdr.fresh_fill || T <= 0 || (T & 63)) return SPICEY_ERR_BAD_DESC;
  if (!spicey_ready_steps_ok(steps)) return SPICEY_ERR_BAD_DESC;  // (the launch would not have chosen either build)
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
  const bool afit = spicey_addr_fits(P, hr.tail_n), ufit = spicey_u0_resident_fits(P, hr.st_desc.data(), T);
  if (info8) {
    const int64_t v[8] = {hr.st_desc[0], hr.st_desc[2], hr.st_desc[5], ufit, P.pcr_n, P.pcr_level, P.nLevels, afit};
    memcpy(info8, v, sizeof(v));
  }
  if (raw) {
    memset(raw, 0, sizeof(uint32_t) * (size_t)T * 8);
    if (hr.st_desc[0] == 1u)
      for (int t = 0; t < T && (uint32_t)t < hr.st_desc[2]; t++) memcpy(raw + (size_t)t * 8, P.fus16 + (size_t)hr.st_desc[1] * 4 + (size_t)t * 8, 32);
  }
  if (!spicey_slots_fit(P, hr.tail_n) || !spicey_pt_runtime_choice(P, Q) || !afit) return SPICEY_ERR_BAD_DESC;  // (the plan would not have chosen either build)
  if (resident && !ufit) return SPICEY_ERR_BAD_DESC;
  for (int g = 0; g < ni; g++) {
    Arena a(P, hr.tail_n, fill, g);
    std::vector<FreshRegs> regs(T);
    if (nan)
      for (FreshRegs &r : regs) {
        for (auto &item : r.pf) for (double &v : item) v = std::numeric_limits<double>::quiet_NaN();
        r.srcn = std::numeric_limits<double>::quiet_NaN();
        for (uint32_t &w : r.u0) w = 0xFFFFFFFFu;
      }
    SeqExecIdle ex;
    ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
    if (resident) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true>(ex, P, Q, R, a.c, g);
    else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, false>(ex, P, Q, R, a.c, g);
    if (u0_out)
      for (int t = 0; t < T; t++) memcpy(u0_out + ((size_t)g * T + t) * 8, regs[t].u0, 32);
  }
  int64_t tot = 0;
  for (int g = 0; g < ni; g++) tot += (int64_t)solves[g];
  if (solves_out) *solves_out = tot;
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) {
      if (err4) memcpy(err4, &status[(size_t)g * 4], 16);
      return SPICEY_ERR_SINGULAR;
    }
  return SPICEY_OK;
}

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there), and what a run of `steps` steps on
// such a handle launches: out12 = {u0_resident, top_regs, addr, packed, fresh, threads, inst_per_wg, spicey_top_regs_run,
// spicey_u0_resident_run, st_desc[0], st_desc[2], st_desc[5]} (the descriptor words: 0 where the plan has no v2 layout)
extern "C" int32_t spicey_u0host_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out12) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  const bool has = hres.st_desc.size() >= 8;
  out12[0] = plan.u0_resident; out12[1] = plan.top_regs; out12[2] = plan.addr; out12[3] = plan.packed; out12[4] = plan.fresh; out12[5] = plan.T; out12[6] = plan.K;
  out12[7] = spicey_top_regs_run(plan, steps); out12[8] = spicey_u0_resident_run(plan, steps);
  out12[9] = has ? hres.st_desc[0] : 0; out12[10] = has ? hres.st_desc[2] : 0; out12[11] = has ? hres.st_desc[5] : 0;
  return SPICEY_OK;
}

// The decision for a SYNTHETIC phase-0 descriptor {rows, first, cnt, rhs, rfirst, rcnt, rrhs} of a fresh-fill program with
// nD diodes and a top of 64 rows at level 2, on build `shape` at T threads of a plan whose `top_regs` is given, knobs from
// the environment.  out4 = {spicey_u0_resident_fits, LaunchPlan::u0_resident, then for a plan with slots, ready and addr
// set: spicey_u0_resident_run (10 000 steps), shape's `u0_resident`}
extern "C" void spicey_u0host_decide(int32_t top_regs, int32_t rows, int32_t cnt, int32_t rcnt, int32_t nD, int32_t T, int32_t shape, int64_t *out4) {
  SpiceyProg P{};
  P.nLevels = 4; P.pcr_n = 64; P.pcr_level = 2; P.fresh_fill = 1; P.nD = nD;
  const uint32_t dsc[8] = {(uint32_t)rows, 0u, (uint32_t)cnt, (uint32_t)cnt, 0u, (uint32_t)rcnt, 0u, 0u};
  LaunchPlan plan;
  plan.slots = true; plan.ready = true; plan.addr = true; plan.top_regs = top_regs != 0;
  plan.u0_resident = spicey_plan_u0_resident(plan.top_regs, P, dsc, T, shape, spicey_read_knobs());
  out4[0] = spicey_u0_resident_fits(P, dsc, T); out4[1] = plan.u0_resident; out4[2] = spicey_u0_resident_run(plan, 10000);
  out4[3] = (shape >= 0 && shape < SPICEY_V2_NSHAPES) ? SPICEY_V2_SHAPES[shape].u0_resident : 0;
}

// the packed fresh shape's index in SPICEY_V2_SHAPES, the packed default shape's, the 1024-thread latency shape's
extern "C" void spicey_u0host_shapes(int32_t *out3) {
  out3[0] = spicey_v2_shape(512, true, false, true);
  out3[1] = spicey_v2_shape(512, true, false, false);
  out3[2] = spicey_v2_shape(1024, false, false, false);
}

// The port of the device library's exp as this compiler builds it (fma, rint, ldexp of the host), and the host's exp
extern "C" void spicey_u0host_exp(const double *x, int64_t n, double *port, double *libm) {
  for (int64_t i = 0; i < n; i++) {
    port[i] = spicey_exp_port(x[i], spicey_exp_tab());
    libm[i] = exp(x[i]);
  }
}
