// tests/fixed_schedule_host/harness.cpp — CPU harness of the fixed schedule: the time loop of the fused build written out
// for what the plan holds (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// operand-address build <4, 2, 2> in its fused form (tran_v2_run.h: SF, as tests/stamp_fuse_host runs it) and in that form's
// fixed schedule (FS).  Every workgroup lives in ONE arena of exactly spicey_lds_bytes bytes, laid out as the kernel lays
// out its LDS, and the parameter record is a heap block of exactly the planned size with the fold's table and the fuse's
// behind it, as the handle keeps them.  Also the launch plan's decision and the predicate by itself.
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
  size_t n;
  double *mem;
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

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d`.  form: 0 = the fused form (the loop that
// decides its schedule in every step), 1 = its fixed schedule — refused (SPICEY_ERR_BAD_DESC) where the fuse does not fit or
// spicey_fixed_schedule_fits says no, as the plan would refuse it.  src: the source table, instance g's at src + g x
// src_stride (0: one for all).  flags bit 0: threads of a phase in reverse order, bit 1: the arena, the parameter record and
// the prefetch registers start as NaN / all ones, bit 2: the executor without idle waves (the early fetch in a phase of its
// own).  err4: the status words {code, inst, step, iter} of the first workgroup that failed.
// info8 = {spicey_fixed_schedule_fits, spicey_stamp_fuse_table, spicey_top_fold_table, nLevels, pcr_level, k_merge, streamed
// phases, pcr_n}.
extern "C" int32_t spicey_fshost_run(const SpiceyDesc *d, int32_t form, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *out_v,
                                     double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags, int64_t *info8,
                                     int32_t *err4, int64_t *solves_out) {
  HostProgram hp;
  std::string err;
  int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return rc;
  if (hp.structurally_singular || !hp.hdr.has16 || !hp.hdr.fresh_fill || T <= 0 || (T & 63)) return SPICEY_ERR_BAD_DESC;
  if (!spicey_ready_steps_ok(steps)) return SPICEY_ERR_BAD_DESC;
  SpiceyProg P = hp.bind(hp.blob.data());
  const int ni = d->n_inst;
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  SpiceyResident Q = hr.bind(hr.blob.data());
  const bool afit = spicey_addr_fits(P, hr.tail_n), ufit = spicey_u0_resident_fits(P, hr.st_desc.data(), T);
  std::vector<uint32_t> table, ftable;
  const bool tfit = ufit && P.pcr_level >= 2 && spicey_top_fold_table(hp, hr.tail_n, table);
  const bool sfit = tfit && spicey_stamp_fuse_table(hp, hr.tail_n, T, 2, 2, ftable);
  const bool fsfit = sfit && spicey_fixed_schedule_fits(hp, hr);
  if (info8) {
    int64_t streamed = 0;
    for (uint32_t c : hr.st_cnt) streamed += c != 0u;
    const int64_t v[8] = {fsfit, sfit, tfit, P.nLevels, P.pcr_level, hr.k_merge, streamed, P.pcr_n};
    memcpy(info8, v, sizeof(v));
  }
  if (!spicey_slots_fit(P, hr.tail_n) || !spicey_pt_runtime_choice(P, Q) || !afit || !sfit) return SPICEY_ERR_BAD_DESC;  // (the plan would not have fused)
  if (form && !fsfit) return SPICEY_ERR_BAD_DESC;
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
  const bool nan = (flags & 2) != 0;
  const double fill = nan ? std::numeric_limits<double>::quiet_NaN() : 0.0;
  // the parameter record, behind it the fold's table, behind that the fuse's: a heap block of exactly that size
  const size_t nz = (size_t)ni * 2 * (size_t)T * 5, nf = SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t) / sizeof(double);
  std::vector<double> zpar(nz + nf + spicey_stamp_fuse_words(T) * sizeof(uint32_t) / sizeof(double), fill);
  memcpy(zpar.data() + nz, table.data(), SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t));
  memcpy(zpar.data() + nz + nf, ftable.data(), ftable.size() * sizeof(uint32_t));
  R.zpar = zpar.data();
  for (int g = 0; g < ni; g++) {
    Arena a(P, hr.tail_n, fill, g);
    std::vector<FreshRegs> regs(T);
    if (nan)
      for (FreshRegs &r : regs) {
        for (auto &item : r.pf) for (double &v : item) v = std::numeric_limits<double>::quiet_NaN();
        r.srcn = std::numeric_limits<double>::quiet_NaN();
        for (uint32_t &w : r.u0) w = 0xFFFFFFFFu;
      }
    if (flags & 4) {
      SeqExec ex;
      ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
      if (form) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true, true, true, true>(ex, P, Q, R, a.c, g);
      else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true, true, true>(ex, P, Q, R, a.c, g);
    } else {
      SeqExecIdle ex;
      ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
      if (form) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true, true, true, true>(ex, P, Q, R, a.c, g);
      else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true, true, true>(ex, P, Q, R, a.c, g);
    }
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
// such a handle launches: out8 = {fixed_schedule, stamp_fuse, top_fold, packed, fresh, threads, spicey_fixed_schedule_run,
// spicey_stamp_fuse_run}
extern "C" int32_t spicey_fshost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out8) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  out8[0] = plan.fixed_schedule; out8[1] = plan.stamp_fuse; out8[2] = plan.top_fold; out8[3] = plan.packed; out8[4] = plan.fresh; out8[5] = plan.T;
  out8[6] = spicey_fixed_schedule_run(plan, steps); out8[7] = spicey_stamp_fuse_run(plan, steps);
  return SPICEY_OK;
}

// The predicate by itself on the packed layout of the fresh-fill program of `d`, and on that layout with one thing changed
// that the written-out loop could not run.  out8 = spicey_fixed_schedule_fits of {the layout as built, one backward phase
// marked streamed, the merged backward phase unmerged, a resident backward record with three products, a factor phase the
// loop runs without tasks, an LDS tail, a top of 65 rows, 0}.  Returns 0, or a negative error code.
extern "C" int32_t spicey_fshost_predicate(const SpiceyDesc *d, int32_t T, int64_t *out8) {
  HostProgram hp;
  std::string err;
  const int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return -rc;
  if (T <= 0 || (T & 63) || !hp.hdr.has16) return -SPICEY_ERR_BAD_DESC;
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  memset(out8, 0, 8 * sizeof(int64_t));
  out8[0] = spicey_fixed_schedule_fits(hp, hr);
  const int nL = hp.hdr.nLevels;
  if (nL <= 0 || (int)hr.st_cnt.size() < 2 * nL) return 0;
  { HostResident h2 = hr; h2.st_cnt[2 * nL - 1] = 1u; out8[1] = spicey_fixed_schedule_fits(hp, h2); }
  { HostResident h2 = hr; h2.k_merge = 0; out8[2] = spicey_fixed_schedule_fits(hp, h2); }
  {
    HostResident h2 = hr;
    const int nW = T / 64;
    bool done = false;
    for (int w = 0; w < nW && !done; w++)
      for (int s = 0; s < h2.rmax && !done; s++)
        if (h2.res_phase[(size_t)w * h2.rmax + s] == 2 * nL - 1) {
          uint32_t &w0 = h2.res[((size_t)s * T + (size_t)w * 64) * 4];
          w0 = (w0 & 0xff00ffffu) | (3u << 16) | ((uint32_t)SPICEY_R16_VALID << 24);
          done = true;
        }
    out8[3] = done ? spicey_fixed_schedule_fits(hp, h2) : -1;
  }
  { HostProgram p2 = hp; if (p2.hdr.pcr_level >= 2) p2.ph_cnt[0] = 0u; out8[4] = spicey_fixed_schedule_fits(p2, hr); }
  { HostResident h2 = hr; h2.tail_n = 3; out8[5] = spicey_fixed_schedule_fits(hp, h2); }
  { HostProgram p2 = hp; p2.hdr.pcr_n = 65; out8[6] = spicey_fixed_schedule_fits(p2, hr); }
  return 0;
}
