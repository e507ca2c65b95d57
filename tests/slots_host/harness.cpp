// tests/slots_host/harness.cpp — CPU harness of the operand-slot builds (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// early-prefetch build <4, 2, 2> with and without the operand slots (tran_pt_layout.h: spicey_slot_index; tran_v2_phases.h: OS).
// The slots are addressed by their index from the start of the workspace, so every run lives in ONE arena of exactly
// spicey_lds_bytes bytes, laid out as the kernel lays out its LDS: workspace, element vectors, switch states and flags,
// profiling slots, tail area.  On request the arena, the record and the prefetch registers start as NaN.  Also the slot
// positions and the launch plan's decision.
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

}  // namespace

// the LDS arena of one workgroup (K = 1, LDS workspace), as spicey_tran_kernel_v2 lays it out
struct SlotsArena {
  std::vector<double> mem;  // (doubles: 8-byte alignment for every section)
  WgCtx<1> c;
  SlotsArena(const SpiceyProg &P, int tail_n, double fill, int inst) {
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

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d` on the early-prefetch build with idle
// waves; slots: 1 = the operand-slot form.  flags bit 0: threads of a phase in reverse order, bit 1: the arena, the record
// and the prefetch registers start as NaN.  info8 = {nV, nS, pcr_n, fresh_fill, spicey_slots_fit, slot index, bit pattern
// of the double at the +0.0 slot after the run, of the one behind it} (the last instance's arena).
extern "C" int32_t spicey_slots_run(const SpiceyDesc *d, int32_t slots, int32_t T, int64_t steps, double dt, const double *src, double *out_v, double *out_i,
                                    int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags, int64_t *info8) {
  HostProgram hp;
  std::string err;
  int32_t rc = spicey_build_program(d, hp, err, true, 0, true, false, true);
  if (rc != SPICEY_OK) return rc;
  if (hp.structurally_singular || !hp.hdr.has16 || !hp.hdr.fresh_fill || T <= 0 || (T & 63)) return SPICEY_ERR_BAD_DESC;
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
  std::vector<double> zpar((size_t)ni * 2 * (size_t)T * 5, fill);
  R.zpar = zpar.data();
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  SpiceyResident Q = hr.bind(hr.blob.data());
  const bool fit = spicey_slots_fit(P, hr.tail_n);
  if (slots && (!fit || !spicey_pt_runtime_choice(P, Q))) return SPICEY_ERR_BAD_DESC;  // (the plan would not have chosen the build)
  const uint32_t zs = spicey_slot_index(P);
  uint64_t bits[2] = {0, 0};
  for (int g = 0; g < ni; g++) {
    SlotsArena a(P, hr.tail_n, fill, g);
    std::vector<FreshRegs> regs(T);
    if (nan)
      for (FreshRegs &r : regs) {
        for (auto &item : r.pf) for (double &v : item) v = std::numeric_limits<double>::quiet_NaN();
        r.srcn = std::numeric_limits<double>::quiet_NaN();
      }
    SeqExecIdle ex;
    ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
    if (slots) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true>(ex, P, Q, R, a.c, g);
    else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, false>(ex, P, Q, R, a.c, g);
    if (fit) memcpy(bits, a.c.W + zs, sizeof(bits));
  }
  if (info8) {
    info8[0] = P.nV; info8[1] = P.nS; info8[2] = P.pcr_n; info8[3] = P.fresh_fill; info8[4] = fit; info8[5] = zs;
    info8[6] = (int64_t)bits[0]; info8[7] = (int64_t)bits[1];
  }
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}

// The slot positions for a program header with these fields (everything else zero): out4 = {spicey_slots_fit, slot index,
// byte offset just behind the -0.0 slot, spicey_lds_bytes of the same header}
extern "C" void spicey_slots_where(int32_t nW, int32_t nU, int32_t nGdyn, int32_t nS, int32_t pcr_n, int32_t pcr_level, int32_t tail_n, int64_t *out4) {
  SpiceyProg P{};
  P.nW = nW; P.nU = nU; P.nGdyn = nGdyn; P.nS = nS; P.pcr_n = pcr_n; P.pcr_level = pcr_level;
  out4[0] = spicey_slots_fit(P, tail_n);
  out4[1] = spicey_slot_index(P);
  out4[2] = ((int64_t)spicey_slot_index(P) + 2) * (int64_t)sizeof(double);
  out4[3] = (int64_t)spicey_lds_bytes(P, 1, true, tail_n);
}

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there): out6 = {slots, early, fresh, packed,
// threads, lds_bytes}
extern "C" int32_t spicey_slots_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t *out6) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  out6[0] = plan.slots; out6[1] = plan.early; out6[2] = plan.fresh; out6[3] = plan.packed; out6[4] = plan.T; out6[5] = (int64_t)plan.lds_bytes;
  return SPICEY_OK;
}
