// tests/addr_host/harness.cpp — CPU harness of the operand-address builds (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and runs the packed layout (T threads, 4 slots) of a fresh-fill program on the fresh
// ready-argument build <4, 2, 2> with and without operand addresses (tran_v2_run.h: OA).  On the host an operand's handle
// is its index from the start of the workspace (tran_common.h: SpiceyOperand), so what runs here is the prologue's
// re-encoding of B's descriptor fields and every read and write through W[field]: every workgroup lives in ONE arena of
// exactly spicey_lds_bytes bytes, laid out as the kernel lays out its LDS, and a field that names a wrong index shows
// as other bits or, past the arena, to the address sanitizer (addr_asan.cpp).  After each instance's run the descriptor
// and terminal registers of every thread are copied out.  Also the fit rule and the launch plan's decision.
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

// One run at the packed layout (T threads, 4 slots) of the fresh-fill program of `d` on the ready-argument build with idle
// waves; addr: 1 = its operand-address form.  src: the source table, instance g's at src + g x src_stride (0: one for all).
// zpar: ni x 2 x T x 5 doubles.  flags bit 0: threads of a phase in reverse order, bit 1: the arena and the prefetch
// registers start as NaN.  regs: ni x T x 14 words, per thread {dd[0], dd[1], rhs[0][0], rhs[0][1], rhs[1][0], rhs[1][1],
// eR[0], eR[1], eC[0], eC[1], eD[0], eD[1], ox[0], ox[1]} after the run.  raw: T x 6 words, the program's own descriptors
// of the same items {ent_dd[tid], ent_dd[tid + T], row_desc[tid][0..1], row_desc[tid + T][0..1]} (0x80000000 / 0xFFFFFFFF
// in the second word: no such entry / row for this thread, as load_resident and a0_initial say it).
// info16 = {nV, nS, pcr_n, fresh_fill, spicey_slots_fit, spicey_addr_fits, nW, nU, nGdyn, spicey_slot_index, nOut, nCur,
// n, nKeep, spicey_addr_max_index, doubles of the arena}.
extern "C" int32_t spicey_oahost_run(const SpiceyDesc *d, int32_t addr, int32_t T, int64_t steps, double dt, const double *src, int64_t src_stride, double *zpar,
                                     double *out_v, double *out_i, int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags,
                                     uint32_t *regs_out, uint32_t *raw, int64_t *info16) {
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
  const bool fit = spicey_slots_fit(P, hr.tail_n), afit = spicey_addr_fits(P, hr.tail_n);
  if (!fit || !spicey_pt_runtime_choice(P, Q)) return SPICEY_ERR_BAD_DESC;  // (the plan would not have chosen either build)
  if (addr && !afit) return SPICEY_ERR_BAD_DESC;
  size_t arena_doubles = 0;
  for (int g = 0; g < ni; g++) {
    Arena a(P, hr.tail_n, fill, g);
    arena_doubles = a.n;
    std::vector<FreshRegs> regs(T);
    if (nan)
      for (FreshRegs &r : regs) {
        for (auto &item : r.pf) for (double &v : item) v = std::numeric_limits<double>::quiet_NaN();
        r.srcn = std::numeric_limits<double>::quiet_NaN();
      }
    SeqExecIdle ex;
    ex.T = T; ex.reverse = (flags & 1) != 0; ex.rr = &regs;
    if (addr) spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, true>(ex, P, Q, R, a.c, g);
    else spicey_tran_run_v2<1, 4, 2, 2, false, -1, true, true, true, false>(ex, P, Q, R, a.c, g);
    if (regs_out)
      for (int t = 0; t < T; t++) {
        const FreshRegs &r = regs[t];
        const uint32_t w[14] = {r.dd[0], r.dd[1], r.rhs[0][0], r.rhs[0][1], r.rhs[1][0], r.rhs[1][1], r.eR[0], r.eR[1], r.eC[0], r.eC[1], r.eD[0], r.eD[1], r.ox[0], r.ox[1]};
        memcpy(regs_out + ((size_t)g * T + t) * 14, w, sizeof(w));
      }
  }
  if (raw)
    for (int t = 0; t < T; t++) {
      uint32_t *w = raw + (size_t)t * 6;
      for (int j = 0; j < 2; j++) {
        const int e = t + j * T;
        w[j] = e < P.nKeep ? P.ent_dd[e] : 0x80000000u;
        w[2 + 2 * j] = e < P.n ? P.row_desc[(size_t)e * 2] : 0u;
        w[3 + 2 * j] = e < P.n ? P.row_desc[(size_t)e * 2 + 1] : 0xFFFFFFFFu;
      }
    }
  if (info16) {
    const int64_t v[16] = {P.nV, P.nS, P.pcr_n, P.fresh_fill, fit, afit, P.nW, P.nU, P.nGdyn, (int64_t)spicey_slot_index(P), P.nOut, P.nCur,
                           P.n, P.nKeep, (int64_t)spicey_addr_max_index(P), (int64_t)arena_doubles};
    memcpy(info16, v, sizeof(v));
  }
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there), and what a run of `steps` steps on
// such a handle launches: out12 = {addr, ready, slots, early, fresh, packed, threads, lds_bytes, spicey_ready_run,
// spicey_addr_run, SpiceyInfo.operand_addr, inst_per_wg}
extern "C" int32_t spicey_oahost_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, int64_t steps, int64_t *out12) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  SpiceyInfo info;
  fill_info(plan, hp, hres, o, &info);
  out12[0] = plan.addr; out12[1] = plan.ready; out12[2] = plan.slots; out12[3] = plan.early; out12[4] = plan.fresh; out12[5] = plan.packed; out12[6] = plan.T;
  out12[7] = (int64_t)plan.lds_bytes; out12[8] = spicey_ready_run(plan, steps); out12[9] = spicey_addr_run(plan, steps); out12[10] = info.operand_addr;
  out12[11] = plan.K;
  return SPICEY_OK;
}

// The fit rule and the plan's decision for a SYNTHETIC program header: a tridiagonal top of pcr_n rows at level pcr_level,
// nW / nU / nGdyn doubles and nS switch states in the workspace, hybrid layout or not; on build `shape` (an index into
// SPICEY_V2_SHAPES) at K instances per workgroup, knobs from the environment.  out8 = {spicey_slots_fit, spicey_addr_fits,
// spicey_addr_max_index, the field's largest value, LaunchPlan::addr, then for a plan with slots and ready set:
// spicey_ready_run, spicey_addr_run (10 000 steps), shape's `addr`}
extern "C" void spicey_oahost_fits(int32_t nW, int32_t nU, int32_t nGdyn, int32_t nS, int32_t pcr_n, int32_t pcr_level, int32_t tail_n, int32_t hybrid, int32_t K,
                                   int32_t shape, int64_t *out8) {
  SpiceyProg P{};
  P.nW = nW; P.nU = nU; P.nGdyn = nGdyn; P.nS = nS; P.pcr_n = pcr_n; P.pcr_level = pcr_level; P.hybrid = hybrid;
  LaunchPlan plan;
  plan.slots = true; plan.ready = true; plan.lds = true; plan.K = K;
  plan.addr = spicey_plan_addr(P, tail_n, K, true, shape, spicey_read_knobs());
  out8[0] = spicey_slots_fit(P, tail_n); out8[1] = spicey_addr_fits(P, tail_n); out8[2] = (int64_t)spicey_addr_max_index(P); out8[3] = SPICEY_ADDR_FIELD_MAX;
  out8[4] = plan.addr; out8[5] = spicey_ready_run(plan, 10000); out8[6] = spicey_addr_run(plan, 10000);
  out8[7] = (shape >= 0 && shape < SPICEY_V2_NSHAPES) ? SPICEY_V2_SHAPES[shape].addr : 0;
}

// the packed fresh shape's index in SPICEY_V2_SHAPES, a hybrid shape's, and the packed default shape's
extern "C" void spicey_oahost_shapes(int32_t *out3) {
  out3[0] = spicey_v2_shape(512, true, false, true);
  out3[1] = spicey_v2_shape(512, false, true, false);
  out3[2] = spicey_v2_shape(512, true, false, false);
}
