// tests/top_fold_host/harness.cpp — CPU harness of the fold of the last factor level into the tridiagonal top (TEST
// INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// operand-address build <4, 2, 2> with the register-exchange-top flag, in the form the plan takes without the fold (the
// resident level-0 record where it fits) and with it (tran_v2_run.h: TF — the host restatement spicey_top_fold_wave runs
// "record, then the stages" for the top's wave).  Every workgroup lives in ONE arena of exactly spicey_lds_bytes bytes, laid
// out as the kernel lays out its LDS (tests/addr_host), and the parameter record is a heap block of exactly the planned
// size with the fold's table behind it, as the handle keeps it.  Also the launch plan's decision and the table itself.
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

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d`.  fold: 0 = the form a plan without the
// fold takes (the resident level-0 record where spicey_u0_resident_fits holds, the fetched one elsewhere), 1 = the fold on
// top of the resident record — refused (SPICEY_ERR_BAD_DESC) where the record does not fit or spicey_top_fold_table says
// no, as the plan would refuse it.  src: the source table, instance g's at src + g x src_stride (0: one for all).
// flags bit 0: threads of a phase in reverse order, bit 1: the arena, the parameter record and the prefetch registers start
// as NaN / all ones.  err4: the status words {code, inst, step, iter} of the first workgroup that failed.
// info8 = {pcr_n, pcr_level, nLevels, row records of level pcr_level - 1, its generic remainder, spicey_top_fold_table,
// spicey_u0_resident_fits, records of the table that have a pivot}.
extern "C" int32_t spicey_tfhost_run(const SpiceyDesc *d, int32_t fold, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *out_v,
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
  std::vector<uint32_t> table;
  const bool tfit = spicey_top_fold_table(hp, hr.tail_n, table);
  if (info8) {
    const int l = P.pcr_level - 1;
    int64_t piv = 0;
    for (size_t i = 0; tfit && i < 64; i++) piv += (table[i * 8] >> 16) & 3u ? 1 : 0;
    const int64_t v[8] = {P.pcr_n, P.pcr_level, P.nLevels, l >= 0 ? hp.fus_pairs[l] : 0, l >= 0 ? hp.fus_gen[l] : 0, tfit, ufit, piv};
    memcpy(info8, v, sizeof(v));
  }
  if (!spicey_slots_fit(P, hr.tail_n) || !spicey_pt_runtime_choice(P, Q) || !afit) return SPICEY_ERR_BAD_DESC;  // (the plan would not have chosen either build)
  if (fold && (!ufit || !tfit)) return SPICEY_ERR_BAD_DESC;
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
  // the parameter record, and behind it the fold's table where the run folds: a heap block of exactly that size
  const size_t nz = (size_t)ni * 2 * (size_t)T * 5;
  std::vector<double> zpar(nz + (fold ? SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t) / sizeof(double) : 0), fill);
  if (fold) memcpy(zpar.data() + nz, table.data(), SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t));
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
    SeqExecIdle ex;
    ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
    if (fold) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true, true>(ex, P, Q, R, a.c, g);
    else if (ufit) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, true, false>(ex, P, Q, R, a.c, g);
    else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true, true, false, false>(ex, P, Q, R, a.c, g);
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
// such a handle launches: out12 = {top_fold, u0_resident, top_regs, addr, packed, fresh, threads, inst_per_wg,
// spicey_top_fold_run, spicey_u0_resident_run, pcr_n, pcr_level}
extern "C" int32_t spicey_tfhost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out12) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  out12[0] = plan.top_fold; out12[1] = plan.u0_resident; out12[2] = plan.top_regs; out12[3] = plan.addr; out12[4] = plan.packed; out12[5] = plan.fresh; out12[6] = plan.T;
  out12[7] = plan.K; out12[8] = spicey_top_fold_run(plan, steps); out12[9] = spicey_u0_resident_run(plan, steps); out12[10] = hp.hdr.pcr_n; out12[11] = hp.hdr.pcr_level;
  return SPICEY_OK;
}

// The fold's table of the fresh-fill program of `d` at the packed layout (T threads): table = SPICEY_TOP_FOLD_WORDS words
// (zeros where there is none), tab = the top's index table [64][4] (0xFFFF beyond pcr_n), rows = the program's row records
// of level pcr_level - 1 [64][8] in the program's order.  info8 as spicey_tfhost_run's; word 7 of it = the +0.0 slot's index.
// Returns spicey_top_fold_table's answer, or a negative error code.
extern "C" int32_t spicey_tfhost_table(const SpiceyDesc *d, int32_t T, uint32_t *table, uint16_t *tab, uint32_t *rows, int64_t *info8) {
  HostProgram hp;
  std::string err;
  const int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return -rc;
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  const SpiceyProg &P = hp.hdr;
  std::vector<uint32_t> t;
  const bool ok = hp.hdr.has16 && spicey_top_fold_table(hp, hr.tail_n, t);
  memset(table, 0, SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t));
  if (ok) memcpy(table, t.data(), SPICEY_TOP_FOLD_WORDS * sizeof(uint32_t));
  for (int i = 0; i < 64 * 4; i++) tab[i] = i < P.pcr_n * 4 && (size_t)i < hp.pcr_tab.size() ? hp.pcr_tab[i] : (uint16_t)0xFFFF;
  memset(rows, 0, (size_t)64 * 8 * sizeof(uint32_t));
  const int l = P.pcr_level - 1;
  const uint32_t nrow = l >= 0 && l < (int)hp.fus_pairs.size() ? hp.fus_pairs[l] : 0u;
  for (uint32_t j = 0; j < nrow && j < 64u; j++) memcpy(rows + (size_t)j * 8, &hp.fus16[((size_t)hp.fus_first[l] + hp.fus_gen[l]) * 4 + (size_t)j * 8], 32);
  const int64_t v[8] = {P.pcr_n, P.pcr_level, P.nLevels, nrow, l >= 0 && l < (int)hp.fus_gen.size() ? hp.fus_gen[l] : 0, ok, spicey_u0_resident_fits(P, hr.st_desc.data(), T),
                        (int64_t)spicey_slot_index(P)};
  memcpy(info8, v, sizeof(v));
  return ok ? 1 : 0;
}
