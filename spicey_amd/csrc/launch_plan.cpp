// launch_plan.cpp — see launch_plan.h.
#include "launch_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "fronts_exec_consts.h"
#include "tran_pt_layout.h"

// LDS scratch of the dense fronts: the widest panel (U rows 16 x ld, L rows (Mp - 16) x 17, the 16 x 16 block of L and
// the reciprocal pivots), which also covers the backward solve's vectors
size_t spicey_front_lds_bytes(const SpiceyProg &P) {
  if (P.nFronts <= 0) return 0;
  return (size_t)SPICEY_FRONT_LDS_DOUBLES * sizeof(double);  // fronts of up to 128 rows live here whole; larger ones stage panels (max_front_mp <= 448)
}

size_t spicey_lds_bytes(const SpiceyProg &P, int K, bool lds, int tail_n) {
  if (!lds) return 64 + spicey_front_lds_bytes(P);
  size_t b = ((size_t)P.nW + P.nU + P.nGdyn) * K * sizeof(double) + ((size_t)P.nS * K + 4) * sizeof(int32_t);
  if (P.hybrid)  // hybrid workspace: leaf-owned entries and the element vectors are in global memory
    b = ((size_t)P.nW - P.hyb_g0 - P.hyb_g2) * K * sizeof(double) + ((size_t)P.nS * K + 4) * sizeof(int32_t);
  b = ((b + 15) & ~size_t(15)) + SPICEY_PH_SLOTS * sizeof(unsigned long long);  // + profiling accumulators
  if (P.pcr_n > 0 && tail_n < 5) tail_n = 5;                                         // tridiagonal top: two 2 KB row buffers + its index table
  b = ((b + 15) & ~size_t(15)) + (size_t)tail_n * 64 * 16;                          // + tail task records
  b += spicey_front_lds_bytes(P);                                                    // + dense-front scratch (32-bit interpreter only)
  return (b + 15) & ~size_t(15);
}

size_t spicey_gw_doubles_per_wg(const SpiceyProg &P, int K) {
  return ((size_t)P.nW + P.nU + P.nGdyn) * K + (((size_t)P.nS * K + 1) >> 1);
}

int spicey_v2_shape(int threads, bool packed, bool hybrid, bool fresh) {
  for (int i = 0; i < SPICEY_V2_NSHAPES; i++) {
    const SpiceyV2Shape &s = SPICEY_V2_SHAPES[i];
    if (s.packed == packed && s.hybrid == hybrid && s.fresh == fresh && threads <= s.threads) return i;
  }
  return -1;
}
// (beyond every build of the kind: the numbers of the widest plain build, the last entry)
static const SpiceyV2Shape &v2_build(int threads, bool packed = false, bool hybrid = false) {
  const int i = spicey_v2_shape(threads, packed, hybrid);
  return SPICEY_V2_SHAPES[i >= 0 ? i : SPICEY_V2_NSHAPES - 1];
}

SpiceyKnobs spicey_read_knobs() {
  const char *ms = getenv("SPICEY_GROUP_TIMEOUT_MS");
  return {getenv("SPICEY_NO_HYBRID") != nullptr, getenv("SPICEY_FRONT_RIGHT_LOOKING") != nullptr, getenv("SPICEY_TEST_FORCE_GROUP_ABORT") != nullptr,
          ms ? atoi(ms) : 0, getenv("SPICEY_NO_PHASE_TABLE") != nullptr, getenv("SPICEY_NO_FRESH_FILL") != nullptr, getenv("SPICEY_FRESH_FILL_LINEAR") != nullptr, getenv("SPICEY_NO_EARLY_PREFETCH") != nullptr, getenv("SPICEY_NO_OPERAND_SLOTS") != nullptr, getenv("SPICEY_NO_READY_ARGS") != nullptr, getenv("SPICEY_NO_OPERAND_ADDR") != nullptr, getenv("SPICEY_NO_TOP_REGS") != nullptr, getenv("SPICEY_NO_U0_RESIDENT") != nullptr, getenv("SPICEY_NO_TOP_FOLD") != nullptr, getenv("SPICEY_NO_STAMP_FUSE") != nullptr, getenv("SPICEY_NO_FIXED_SCHEDULE") != nullptr};
}

static int pick_threads(const HostProgram &hp, bool v2) {
  const SpiceyProg &P = hp.hdr;
  if (v2) {
    // smallest workgroup in which the whole program is register-resident: all factor/backward tasks in the
    // RMAX slots, one right-hand-side row, one element of each kind and NSV re-stamped entries per thread
    int64_t chunks = 0;  // 64-lane chunks of task records
    for (uint32_t c : hp.ph_cnt) chunks += (c + 63) / 64;
    const int widest = std::max(std::max(P.n, P.nOut), std::max(std::max(P.nR, P.nC), P.nD));
    // measured on diode_chain(1000): per-step time T=1024 < T=512 < T=256 (more waves hide the issue-bound
    // phases B/Z); small circuits take the smallest workgroup that holds everything
    const int tmax = SPICEY_V2_SHAPES[SPICEY_V2_NSHAPES - 1].threads;  // (v2 runs one instance per workgroup)
    for (int T = 64; T <= tmax; T *= 2) {
      const SpiceyV2Shape &b = v2_build(T);
      const bool fits = chunks <= (int64_t)b.rmax * (T / 64) && widest <= b.nel * T && P.nRestore <= b.nsv * T;
      if (fits && (T >= tmax || widest <= T)) return T;  // prefer one element per thread when a larger T offers it
    }
    return tmax;
  }
  const int n = P.n;
  if (n <= 48) return 64;
  if (n <= 160) return 128;
  if (n <= 400) return 256;
  if (n <= 4000) return 512;
  return 1024;
}

SpiceyExactWs spicey_exact_ws(const SpiceyDesc &d) {
  SpiceyExactWs w{};
  const int64_t n = (int64_t)d.n_nodes + d.nV;
  w.ld = (int32_t)((n + 1) | 1);
  w.mw = (int32_t)((n + 31) / 32);
  int32_t o = 0;
  auto slots = [&](int32_t &at, int32_t cnt) { at = o; o += cnt; };
  slots(w.qR, d.nR); slots(w.qGc, d.nC); slots(w.qIc, d.nC); slots(w.qGl, d.nL); slots(w.qIl, d.nL);
  slots(w.qS, d.nS); slots(w.qV, d.nV); slots(w.qGd, d.nD); slots(w.qIeq, d.nD); slots(w.qOne, 1);
  w.nq = o;
  int64_t at = 0;
  auto carve = [&](int64_t &off, int64_t doubles) { off = at; at += doubles; };
  carve(w.A, n * w.ld); carve(w.x, n); carve(w.q, w.nq); carve(w.vdlin, d.nD); carve(w.act_f, n);
  carve(w.perm, (n + 1) / 2); carve(w.act_r, (n + 1) / 2); carve(w.mask, (n * w.mw + 1) / 2);
  w.doubles = (at + 1) & ~int64_t(1);  // (16-byte multiple: the next instance's slab stays aligned)
  return w;
}

// interpreter 3: the reference-order engine (exact_exec.h).  Sizes and options only; no symbolic program, no structural
// pre-check (the reference throws only where its own pivot search does).
static int32_t plan_exact(const SpiceyDesc *desc, const SpiceyOptions &opt, const PlanDevice &dev, HostProgram &hp, LaunchPlan &plan,
                          std::string &err) {
  auto fail = [&](int32_t code, const char *msg) { err = msg; return code; };
  int32_t rc = spicey_check_desc(desc, err);
  if (rc != SPICEY_OK) return rc;
  if (opt.inst_per_wg > 1) return fail(SPICEY_ERR_BAD_DESC, "interpreter 3 (reference order) runs one instance per workgroup: inst_per_wg must be 0 or 1");
  if (opt.geometry != 0) return fail(SPICEY_ERR_BAD_DESC, "interpreter 3 (reference order) has no geometry option: geometry must be 0");
  if (opt.front_cut > 0) return fail(SPICEY_ERR_BAD_DESC, "interpreter 3 (reference order) has no dense fronts: front_cut must be <= 0");
  if (opt.wgs_per_inst > 1) return fail(SPICEY_ERR_BAD_DESC, "interpreter 3 (reference order) runs one workgroup per instance: wgs_per_inst must be 0 or 1");
  if (opt.profile) return fail(SPICEY_ERR_BAD_DESC, "interpreter 3 (reference order) has no phase profile: profile must be 0");
  if (opt.threads != 0 && (opt.threads > 1024 || opt.threads < 64 || (opt.threads & 63)))
    return fail(SPICEY_ERR_BAD_DESC, "threads must be a multiple of 64 in [64, 1024]");
  SpiceyProg &P = hp.hdr;
  P.n = desc->n_nodes + desc->nV;
  P.nR = desc->nR; P.nC = desc->nC; P.nL = desc->nL; P.nV = desc->nV; P.nS = desc->nS; P.nD = desc->nD;
  P.nOut = (desc->n_out > 0 && desc->out_nodes) ? desc->n_out : desc->n_nodes;
  P.nCur = P.nR + P.nC + P.nL + P.nV + P.nS + P.nD;
  if ((int64_t)P.n * ((P.n + 1) | 1) >= ((int64_t)1 << 32)) return fail(SPICEY_ERR_BAD_DESC, "interpreter 3 (reference order): n x (n + 1) must stay below 2^32 entries");
  int ncu = 256;
  if ((rc = dev.open(opt.device, &ncu, err)) != SPICEY_OK) return rc;
  plan.n_inst = desc->n_inst;
  plan.interp = 3;
  plan.K = 1;
  plan.G = 1;
  plan.grid = desc->n_inst;
  // 64 threads up to n = 64 (one wave: its barriers cost next to nothing), 256 above
  plan.T = opt.threads > 0 ? opt.threads : (P.n <= 64 ? 64 : 256);
  plan.xws = spicey_exact_ws(*desc);
  const size_t bytes = (size_t)plan.xws.doubles * sizeof(double);
  plan.lds = !opt.force_global && bytes + SPICEY_EXACT_STATIC_LDS <= SPICEY_LDS_MAX;
  plan.lds_bytes = plan.lds ? bytes : 0;
  return SPICEY_OK;
}

SpiceyAcExactWs spicey_ac_exact_ws(const SpiceyDesc &d) {
  SpiceyAcExactWs w{};
  const int64_t n = (int64_t)d.n_nodes + d.nV;
  w.ld = (int32_t)((n + 1) | 1);
  int32_t o = 0;
  auto slots = [&](int32_t &at, int32_t cnt) { at = o; o += cnt; };
  slots(w.qR, d.nR); slots(w.qC, d.nC); slots(w.qL, d.nL); slots(w.qV, d.nV); slots(w.qOne, 1);
  w.nq = o;
  int64_t at = 0;
  auto carve = [&](int64_t &off, int64_t cx) { off = at; at += cx; };
  carve(w.A, n * w.ld); carve(w.x, n); carve(w.q, w.nq); carve(w.f, n); carve(w.perm, (n + 3) / 4); carve(w.act, (n + 3) / 4);
  w.cx = at;
  return w;
}

// interpreter 3 of an AC handle: sizes and threads only; no sparse program, no structural pre-check (the reference throws
// only where its own pivot search or divisions do)
int32_t spicey_ac_exact_plan(const SpiceyDesc *desc, const SpiceyOptions &opt, AcExactPlan &plan, std::string &err) {
  SpiceyDesc d = *desc;  // simulateAC.ts:38-59 stamps R, C, L and V only
  d.nS = 0;
  d.nD = 0;
  int32_t rc = spicey_check_desc(&d, err);
  if (rc != SPICEY_OK) return rc;
  if (opt.threads != 0 && (opt.threads > 1024 || opt.threads < 64 || (opt.threads & 63))) {
    err = "threads must be a multiple of 64 in [64, 1024]";
    return SPICEY_ERR_BAD_DESC;
  }
  const int64_t n = (int64_t)d.n_nodes + d.nV;
  if (n * ((n + 1) | 1) >= ((int64_t)1 << 32)) {
    err = "interpreter 3 (reference order): n x (n + 1) must stay below 2^32 entries";
    return SPICEY_ERR_BAD_DESC;
  }
  // 64 threads up to n = 64 (one wave: the pivot search needs no barrier), 256 above
  plan.T = opt.threads > 0 ? opt.threads : (n <= 64 ? 64 : 256);
  plan.ws = spicey_ac_exact_ws(d);
  const size_t bytes = (size_t)plan.ws.cx * 16;
  plan.lds = !opt.force_global && bytes + SPICEY_AC_EXACT_STATIC_LDS <= SPICEY_LDS_MAX;
  plan.lds_bytes = plan.lds ? bytes : 0;
  return SPICEY_OK;
}

int64_t spicey_ac_exact_chunk(const AcExactPlan &plan, int64_t slots) {
  if (plan.lds || slots <= 0) return slots;
  return std::min<int64_t>(slots, std::max<int64_t>(1, SPICEY_AC_EXACT_SLAB_MAX / (plan.ws.cx * 16)));
}

int32_t spicey_plan(const SpiceyDesc *desc, const SpiceyOptions &opt, const SpiceyKnobs &knobs, const PlanDevice &dev, HostProgram &hp,
                    HostResident &hres, LaunchPlan &plan, std::string &err) {
  if (opt.interpreter == 3) return plan_exact(desc, opt, dev, hp, plan, err);
  auto fail = [&](int32_t code, const char *msg) { err = msg; return code; };
  // dense fronts: explicit level, or automatic for large nonlinear circuits that run one instance per workgroup (the
  // interleaved K > 1 layouts and forced interpreter 2 keep the task lists); -1 = never
  int front_cut = opt.front_cut > 0 ? opt.front_cut : (opt.front_cut == 0 ? -1 : 0);
  if (opt.inst_per_wg > 1 || opt.interpreter == 2) front_cut = 0;
  if (front_cut < 0 && desc && desc->n_inst >= 512) front_cut = 0;  // big batches fill the chip with interleaved instances instead
  // tridiagonal top by cyclic reduction (16-bit records, one instance per workgroup); diagnostics: bit 5 = never
  const bool pcr_top = !((opt.debug >> 5) & 1) && opt.inst_per_wg <= 1;
  const bool bank_aware = !((opt.debug >> 2) & 1);  // diagnostics: bit 2 = plain CSR numbering
  int32_t rc = spicey_build_program(desc, hp, err, bank_aware, front_cut, pcr_top);
  if (rc != SPICEY_OK) return rc;
  plan.n_inst = desc->n_inst;
  plan.algo_bytes = spicey_algorithmic_bytes(desc, hp.nnzA, hp.hdr.nLU);
  int ncu = 256;
  if ((rc = dev.open(opt.device, &ncu, err)) != SPICEY_OK) return rc;

  // ---- geometry: instances per workgroup, threads, LDS or global workspace --------------------
  const SpiceyProg &P = hp.hdr;  // (follows hp through the hybrid rebuild)
  int K = opt.inst_per_wg;
  const bool want_lds = !opt.force_global;
  if (K != 0 && K != 1 && K != 2 && K != 4) return fail(SPICEY_ERR_BAD_DESC, "inst_per_wg must be 0, 1, 2 or 4");
  // diagnostics are compiled into the kernels with at most two interleaved instances and not into the two-workgroups-per-CU
  // geometry (tran_exec.h, DIAG): a handle with the option stays out of both
  const bool diag = opt.diagnostics != 0;
  if (diag && (K == 4 || opt.geometry == 2)) return fail(SPICEY_ERR_BAD_DESC, "diagnostics need inst_per_wg <= 2 and geometry != 2");
  if (P.nS > 0) K = 1;  // the switch iteration count is per instance: no interleaving
  if (P.nFronts > 0) K = 1;  // dense fronts: one instance per workgroup (group)
  if (K == 0) {
    // LDS path: one instance per workgroup (measured faster than two interleaved ones: VGPR pressure in phase Z).
    // Global-workspace path (large circuits): once the batch exceeds the CUs, interleaving 2-4 instances shares
    // the index stream and fills more of every gathered cache line (rcd_mesh(50) x 1024: ~3x with K = 4).
    K = 1;
    if (!want_lds || spicey_lds_bytes(P, 1, true) > SPICEY_LDS_MAX) K = (plan.n_inst >= 4 * ncu && !diag) ? 4 : (plan.n_inst >= 2 * ncu ? 2 : 1);
  }
  if (K > plan.n_inst) K = 1;
  // Hybrid workspace (program.h, SpiceyProg::hybrid): a circuit whose L+U no longer fits the LDS of one CU but whose upper
  // elimination tree does keeps the 16-bit register-resident interpreter — the entries the LEAVES own (half of L+U under
  // nested dissection) and the element vectors move to global memory, read by one factor phase and one backward phase.
  // Without it such a circuit falls to the 32-bit task lists on a global workspace (diode_chain(2600): 56 us per step on 16
  // cooperating workgroups against ~16 for the 2000-node chain that still fits).  One instance per workgroup; 1024 threads
  // (SpiceyOptions.threads = 512 selects the 512-thread build of the same kernel).
  if (want_lds && (opt.inst_per_wg == 0 || opt.inst_per_wg == 1) && opt.interpreter != 1 && opt.geometry != 2 && P.has16 && P.nFronts == 0 &&
      (opt.threads == 0 || opt.threads == 512 || opt.threads == 1024) && opt.wgs_per_inst <= 1 && !diag && !knobs.no_hybrid &&
      spicey_lds_bytes(P, 1, true, 5) > SPICEY_LDS_MAX) {
    HostProgram hyb;
    std::string err2;
    if (spicey_build_program(desc, hyb, err2, true, 0, pcr_top, true) == SPICEY_OK && hyb.hdr.hybrid && !hyb.ph_cnt.empty() && hyb.ph_cnt[0] > 64 &&
        spicey_lds_bytes(hyb.hdr, 1, true, 5) <= SPICEY_LDS_MAX) {
      hp = std::move(hyb);
      K = 1;
    }
  }
  plan.lds = want_lds && spicey_lds_bytes(P, K, true) <= SPICEY_LDS_MAX;
  if (!plan.lds && want_lds && K > 1 && spicey_lds_bytes(P, 1, true) <= SPICEY_LDS_MAX) {
    K = 1;  // one instance fits LDS where K interleaved ones do not: LDS wins
    plan.lds = true;
  }
  plan.K = K;
  // interpreter: v2 needs the LDS workspace, 16-bit records and one instance per workgroup (the K = 2 build of the
  // register-resident kernel spilled vector registers whatever its geometry: kernels.hip)
  const bool v2_ok = plan.lds && P.has16 && K == 1;
  if (opt.interpreter == 2 && !v2_ok) return fail(SPICEY_ERR_BAD_DESC, "interpreter 2 needs the LDS workspace, < 65536 workspace entries and inst_per_wg = 1");
  plan.interp = (opt.interpreter == 1 || !v2_ok) ? 1 : 2;
  plan.T = opt.threads > 0 ? opt.threads : pick_threads(hp, plan.interp == 2);
  if (P.hybrid) {
    if (plan.interp != 2) return fail(SPICEY_ERR_BAD_DESC, "internal: hybrid layout without the 16-bit interpreter");
    plan.T = opt.threads == 512 ? 512 : 1024;  // (the two geometries the hybrid kernel is built for: SPICEY_V2_SHAPES)
  }
  if (P.nFronts > 0 && plan.T > 512) {  // kernels with the dense-front code are built for <= 512 threads (256 VGPRs)
    if (opt.threads > 512) return fail(SPICEY_ERR_BAD_DESC, "front_cut needs threads <= 512");
    plan.T = 512;
  }
  if (plan.T > 1024 || (plan.T & 63) || plan.T < 64) return fail(SPICEY_ERR_BAD_DESC, "threads must be a multiple of 64 in [64, 1024]");
  plan.grid = (plan.n_inst + K - 1) / K;
  plan.lds_bytes = spicey_lds_bytes(P, K, plan.lds);
  if (plan.interp == 2) {
    // geometry: "throughput" packs two 512-thread workgroups on a CU (needs K = 1, half the LDS, and the per-thread
    // resident items of a 512-thread workgroup); chosen automatically once the batch can fill every CU twice
    const size_t base = spicey_lds_bytes(P, K, true, 0);
    const int widest = std::max(std::max(P.n, P.nOut), std::max(std::max(P.nR, P.nC), P.nD));
    const bool packable = K == 1 && base <= SPICEY_LDS_MAX / 2 && widest <= v2_build(512, true).nel * 512 &&
                          P.nRestore <= v2_build(512, true).nsv * 512 && (opt.threads == 0 || opt.threads == 512);
    if (opt.geometry == 2 && !packable) return fail(SPICEY_ERR_BAD_DESC, "geometry 2 needs inst_per_wg = 1, <= 80 KB of LDS per instance and <= 1024 unknowns");
    if (opt.geometry < 0 || opt.geometry > 2) return fail(SPICEY_ERR_BAD_DESC, "geometry must be 0, 1 or 2");
    plan.packed = packable && !diag && !P.hybrid && (opt.geometry == 2 || (opt.geometry == 0 && plan.n_inst >= 2 * ncu && opt.threads == 0));
    if (plan.packed) plan.T = 512;
    // The packed geometry runs a FRESH-FILL program (program.h: nKeep) on the build made for it where the entries phase B
    // still restores — the kept ones, the dynamic ones among them — fit its two per thread.  Geometry and threads were
    // decided above on nRestore, which the option does not move; nor does it move the records' order, so the resident
    // layout below is the default program's.  A linear circuit keeps the default program: its matrix is stamped and
    // factored once per run (factor reuse), so the re-stamping that the fresh class saves does not happen there.
    const bool linear = P.nD == 0 && P.nS == 0 && P.nDynEnt == 0;
    if (plan.packed && !knobs.no_fresh_fill && (!linear || knobs.fresh_fill_linear)) {
      const SpiceyV2Shape &fs = SPICEY_V2_SHAPES[spicey_v2_shape(plan.T, true, false, true)];
      HostProgram fp;
      std::string err2;
      if (spicey_build_program(desc, fp, err2, bank_aware, front_cut, pcr_top, false, true) == SPICEY_OK && fp.hdr.has16 && fp.hdr.fresh_fill &&
          !fp.structurally_singular && fp.hdr.nRestore == P.nRestore && fp.hdr.nW == P.nW && fp.hdr.nKeep <= fs.nsv * plan.T &&
          fp.hdr.nDynEnt <= fs.nsv * plan.T) {
        hp = std::move(fp);
        plan.fresh = true;
      }
    }
    // tail levels go to LDS: as many as fit beside the workspace (1 KB each), at most 24; the packed geometry
    // must leave room for a second workgroup on the CU
    const size_t lds_cap = plan.packed ? SPICEY_LDS_MAX / 2 : SPICEY_LDS_MAX;
    int max_tail = (int)std::min<size_t>(24, base < lds_cap ? (lds_cap - base) / 1024 : 0);
    if (opt.debug & 1) max_tail = 0;  // diagnostics: disable the tail merge
    spicey_build_resident(hp, plan.T, v2_build(plan.T, plan.packed, P.hybrid != 0).rmax, hres, max_tail, !((opt.debug >> 6) & 1));  // diagnostics: bit 6 = no row records
    plan.lds_bytes = spicey_lds_bytes(P, K, true, hres.tail_n);
    // (the build the launch will pick — spicey_launch_tran_v2 — and whether it has an early-prefetch form)
    const int shape = K == 1 ? spicey_v2_shape(plan.T, plan.packed, hp.hdr.hybrid != 0, plan.packed && hp.hdr.fresh_fill != 0) : -1;
    plan.early = shape >= 0 && SPICEY_V2_SHAPES[shape].early && !knobs.no_early_prefetch;
    // (its operand-slot form needs the phase table and four free words behind it, within reach of a 16-bit index)
    plan.slots = plan.early && SPICEY_V2_SHAPES[shape].slots && !knobs.no_operand_slots && !knobs.no_phase_table && spicey_slots_fit(hp.hdr, hres.tail_n);
    plan.ready = plan.slots && SPICEY_V2_SHAPES[shape].ready && !knobs.no_ready_args;
    // (operand addresses: c.W must be LDS address 0 — one instance per workgroup on the LDS workspace, no hybrid layout — and
    // the re-encoded descriptor fields must hold the largest index, tran_pt_layout.h)
    plan.addr = spicey_plan_addr(hp.hdr, hres.tail_n, K, plan.lds, shape, knobs);
    // (the register-exchange top: the unrolled top of an operand-address run, 1 .. 6 stages)
    plan.top_regs = spicey_plan_top_regs(plan.addr, hp.hdr.pcr_n, shape, knobs);
    // (the resident level-0 record: level 0 streamed as row records, at most one per thread, and nothing else)
    plan.u0_resident = spicey_plan_u0_resident(plan.top_regs, hp.hdr, hres.st_desc.data(), plan.T, shape, knobs);
    // (the fold of the last factor level into the top: that level is row records of the top's rows and nothing else)
    plan.top_fold = spicey_plan_top_fold(plan.u0_resident, hp, hres.tail_n, shape, knobs);
    // (the stamp fuse: every sum of phase B draws on values of one thread of Z)
    plan.stamp_fuse = spicey_plan_stamp_fuse(plan.top_fold, hp, hres.tail_n, plan.T, shape, knobs);
    // (the fixed schedule: every phase but level 0 resident, inline records only, the first backward phase in the top's wave)
    plan.fixed_schedule = spicey_plan_fixed_schedule(plan.stamp_fuse, hp, hres, shape, opt.debug >> 8, knobs);
  }
  if (!plan.lds) {
    // group mode: several CUs per instance when the batch leaves CUs idle and the circuit is large enough for the
    // cross-workgroup barrier (~3 us per phase) to pay; all workgroups must be co-resident: grid * G <= #CU
    int G = opt.wgs_per_inst;
    if (G < 0 || G > 256 || (G > 1 && K > 2)) return fail(SPICEY_ERR_BAD_DESC, "wgs_per_inst must be in [0, 256] (and inst_per_wg <= 2 with it)");
    if (G == 0) {
      G = 1;
      // (with dense fronts the group barriers that are left belong to a dozen wide levels, and the front tree wants one
      // workgroup per subtree: up to 128 CUs for a single instance (measured on rcd_mesh(100): 32 / 48 / 64 / 96 / 128
      // workgroups = 0.78 / 0.71 / 0.70 / 0.69 / 0.68 ms per step); without them every one of ~600 barriers per step grows with G)
      const int gmax = P.nFronts > 0 ? 128 : 16;
      // (the workspace is in HBM / L2 here: from ~10 k entries on (what no longer fits LDS) the extra CUs pay for the group barriers also without
      // fronts — one diode_chain(4000) 68 -> 60 us per step, (8000) 119 -> 77, rc_ladder(8000) 80 -> 66 at G = 16)
      if (K <= 2 && (P.nLU >= 10000 || P.nFronts > 0))
        while (G * 2 <= gmax && plan.grid * G * 2 <= ncu) G *= 2;
    }
    if (plan.grid * G > ncu) G = std::max(1, ncu / plan.grid);
    if (G > 1) {
      // residency: ask the runtime how many workgroups of THIS kernel (its LDS size, these threads) a CU holds; the group
      // is laid out for one per CU, so any answer >= 1 means grid * G <= #CU workgroups are co-resident on an idle device
      const int T_grp = (P.nFronts > 0 && plan.T > 512) ? 512 : plan.T;
      if (dev.grp_blocks_per_cu(P, K, T_grp) < 1) {
        if (opt.wgs_per_inst > 1) return fail(SPICEY_ERR_HIP, "wgs_per_inst: the group-mode kernel cannot be resident on this device (occupancy query says 0 workgroups per CU)");
        G = 1;
      }
    }
    plan.G = G;
  }
  return SPICEY_OK;
}

bool spicey_plan_addr(const SpiceyProg &P, int tail_n, int K, bool lds, int shape, const SpiceyKnobs &knobs) {
  return K == 1 && lds && shape >= 0 && shape < SPICEY_V2_NSHAPES && SPICEY_V2_SHAPES[shape].addr && !SPICEY_V2_SHAPES[shape].hybrid && !P.hybrid &&
         !knobs.no_operand_addr && spicey_addr_fits(P, tail_n);
}
bool spicey_ready_run(const LaunchPlan &plan, int64_t steps) { return plan.slots && plan.ready && spicey_ready_steps_ok(steps); }
bool spicey_addr_run(const LaunchPlan &plan, int64_t steps) { return plan.addr && spicey_ready_run(plan, steps); }
bool spicey_plan_top_regs(bool addr, int pcr_n, int shape, const SpiceyKnobs &knobs) {
  const int S = spicey_top_stages(pcr_n);
  return addr && shape >= 0 && shape < SPICEY_V2_NSHAPES && SPICEY_V2_SHAPES[shape].top_regs && S >= 1 && S <= 6 && !knobs.no_top_regs;
}
bool spicey_top_regs_run(const LaunchPlan &plan, int64_t steps) { return plan.top_regs && spicey_addr_run(plan, steps); }
bool spicey_u0_resident_fits(const SpiceyProg &P, const uint32_t *st_desc, int T) {
  const bool linear = P.nD == 0 && P.nS == 0 && P.nDynEnt == 0;
  return st_desc != nullptr && P.nLevels > 0 && P.pcr_n > 0 && P.pcr_level > 0 && !P.hybrid && P.fresh_fill != 0 && !linear && st_desc[0] == 1u && st_desc[2] >= 1u &&
         st_desc[2] <= (uint32_t)T && st_desc[5] == 0u && st_desc[6] == 0u;
}
bool spicey_plan_u0_resident(bool top_regs, const SpiceyProg &P, const uint32_t *st_desc, int T, int shape, const SpiceyKnobs &knobs) {
  return top_regs && shape >= 0 && shape < SPICEY_V2_NSHAPES && SPICEY_V2_SHAPES[shape].u0_resident && T == SPICEY_V2_SHAPES[shape].threads && !knobs.no_u0_resident &&
         spicey_u0_resident_fits(P, st_desc, T);
}
bool spicey_u0_resident_run(const LaunchPlan &plan, int64_t steps) { return plan.u0_resident && spicey_top_regs_run(plan, steps); }

bool spicey_top_fold_table(const HostProgram &hp, int tail_n, std::vector<uint32_t> &table) {
  table.clear();
  const SpiceyProg &P = hp.hdr;
  const bool linear = P.nD == 0 && P.nS == 0 && P.nDynEnt == 0;
  if (!P.has16 || P.hybrid || !P.fresh_fill || linear || P.pcr_n <= 0 || P.pcr_n > 64 || P.pcr_level < 1 || !spicey_slots_fit(P, tail_n)) return false;
  const int l = P.pcr_level - 1, n = P.pcr_n;
  if (l >= (int)hp.ph_cnt.size() || hp.ph_cnt[l] == 0u || hp.pcr_tab.size() < (size_t)n * 4) return false;
  if (((size_t)hp.ph_first[l] + hp.ph_cnt[l]) * 4 > hp.rec16.size()) return false;
  const uint32_t none = 0xFFFFu, zs = spicey_slot_index(P);
  // the level's tasks by top row and target: [0] sub-diagonal, [1] diagonal, [2] super-diagonal, [3] right-hand side
  struct Task { bool have = false, fresh = false; uint32_t cnt = 0, ldu[2][3] = {}; };
  std::vector<Task> task((size_t)n * 4);
  for (uint32_t j = 0; j < hp.ph_cnt[l]; j++) {
    const uint32_t *w = &hp.rec16[((size_t)hp.ph_first[l] + j) * 4];
    const uint32_t tgt = w[0] & 0xffffu, cnt = (w[0] >> 16) & 0xffu, flags = w[0] >> 24;
    if (!(flags & SPICEY_R16_VALID) || (flags & (SPICEY_R16_RECIP | SPICEY_R16_K)) || cnt < 1u || cnt > 2u || tgt == none) return false;
    int at = -1;
    for (int i = 0; i < n * 4; i++)
      if (hp.pcr_tab[i] == tgt) { if (at >= 0) return false; at = i; }
    if (at < 0 || task[at].have) return false;  // (a target outside the top, or a second task on one target)
    Task &t = task[at];
    t.have = true; t.fresh = (flags & SPICEY_R16_FRESH) != 0; t.cnt = cnt;
    t.ldu[0][0] = w[1] & 0xffffu; t.ldu[0][1] = w[1] >> 16; t.ldu[0][2] = w[2] & 0xffffu;
    t.ldu[1][0] = w[2] >> 16; t.ldu[1][1] = w[3] & 0xffffu; t.ldu[1][2] = w[3] >> 16;
  }
  std::vector<uint16_t> rec((size_t)64 * 16, 0);
  for (int i = 0; i < n; i++) {
    const uint16_t *tb = &hp.pcr_tab[(size_t)i * 4];
    const Task &ts = task[(size_t)i * 4], &td = task[(size_t)i * 4 + 1], &tp = task[(size_t)i * 4 + 2], &ty = task[(size_t)i * 4 + 3];
    uint16_t *r = &rec[(size_t)i * 16];
    if (tb[0] != none && tb[0] == tb[2]) return false;
    if (!td.have && !ty.have && !ts.have && !tp.have) {  // the level does not touch this row: its entries as they stand
      r[0] = tb[1]; r[1] = (uint16_t)(SPICEY_R16_VALID << 8); r[2] = tb[3];
      r[8] = tb[0] != none ? tb[0] : (uint16_t)zs; r[14] = tb[2] != none ? tb[2] : (uint16_t)zs;
      continue;
    }
    // the diagonal's and the right-hand side's task run over the same pivots in the same order, with the same L_ik and d_k
    if (!td.have || !ty.have || td.cnt != ty.cnt || ty.fresh) return false;
    const uint32_t piv = td.cnt;
    for (uint32_t q = 0; q < piv; q++)
      if (td.ldu[q][0] != ty.ldu[q][0] || td.ldu[q][1] != ty.ldu[q][1]) return false;
    if (piv == 2u && td.ldu[0][1] == td.ldu[1][1]) return false;
    // a fill is one product with the L_ik and d_k of one of those pivots
    int of[2] = {-1, -1};  // which side (0 sub, 2 super) pivot q's fill targets
    for (int side : {0, 2}) {
      const Task &tf = side ? tp : ts;
      if (!tf.have) continue;
      if (tf.cnt != 1u) return false;
      int q = -1;
      for (uint32_t k = 0; k < piv; k++)
        if (tf.ldu[0][0] == td.ldu[k][0] && tf.ldu[0][1] == td.ldu[k][1]) q = (int)k;
      if (q < 0 || of[q] >= 0) return false;
      of[q] = side;
    }
    const bool sup0 = of[0] >= 0 ? of[0] == 2 : (of[1] >= 0 ? of[1] == 0 : false);  // pivot 0's side is the super-diagonal
    const int side_of[2] = {sup0 ? 2 : 0, sup0 ? 0 : 2};
    uint32_t meta = piv | ((SPICEY_R16_VALID | SPICEY_R16_FUSED) << 8);
    r[0] = td.fresh ? (uint16_t)zs : tb[1];
    if (td.fresh) meta |= SPICEY_ROW_FRESH_AII;
    r[2] = tb[3];
    for (uint32_t q = 0; q < 2; q++) {
      uint16_t *f = r + 3 + 6 * q;  // L_ik, d_k, U_ki, y_k, U_k,o, where the side starts from
      const Task &tf = side_of[q] ? tp : ts;
      const uint32_t nb = tb[side_of[q]];
      if (q < piv) { f[0] = (uint16_t)td.ldu[q][0]; f[1] = (uint16_t)td.ldu[q][1]; f[2] = (uint16_t)td.ldu[q][2]; f[3] = (uint16_t)ty.ldu[q][2]; }
      if (q < piv && of[q] >= 0) {
        f[4] = (uint16_t)tf.ldu[0][2];
        f[5] = tf.fresh ? (uint16_t)zs : (uint16_t)nb;
        meta |= 1u << (4 + q);
        if (tf.fresh) meta |= q == 0 ? SPICEY_ROW_FRESH_O0 : SPICEY_ROW_FRESH_O1;
      } else {
        f[5] = nb != none ? (uint16_t)nb : (uint16_t)zs;
      }
    }
    r[1] = (uint16_t)meta;
    r[15] = sup0 ? 1u : 0u;
  }
  // nothing behind the top reads what the fold keeps out of W
  std::vector<char> kept((size_t)P.nW + 1, 0);
  for (int i = 0; i < n; i++)
    for (int q = 0; q < 3; q++)
      if (hp.pcr_tab[(size_t)i * 4 + q] != none && hp.pcr_tab[(size_t)i * 4 + q] < (uint32_t)P.nW) kept[hp.pcr_tab[(size_t)i * 4 + q]] = 1;
  auto reads = [&](uint32_t idx) { return idx < kept.size() && kept[idx]; };
  for (int p = P.nLevels; p < 2 * P.nLevels && p < (int)hp.ph_cnt.size(); p++)
    for (uint32_t j = 0; j < hp.ph_cnt[p]; j++) {
      const uint32_t *w = &hp.rec16[((size_t)hp.ph_first[p] + j) * 4];
      const uint32_t cnt = (w[0] >> 16) & 0xffu;
      if (reads(w[1] & 0xffffu)) return false;
      if (cnt <= 2) {
        if ((cnt >= 1 && reads(w[1] >> 16)) || (cnt == 2 && reads(w[2] >> 16))) return false;
      } else {
        for (uint32_t k = 0; k < cnt; k++)
          if ((size_t)w[3] + 2 * k >= hp.ovf16.size() || reads(hp.ovf16[(size_t)w[3] + 2 * k])) return false;
      }
    }
  table.assign(SPICEY_TOP_FOLD_WORDS, 0u);
  memcpy(table.data(), rec.data(), (size_t)64 * 32);
  return true;
}
bool spicey_plan_top_fold(bool u0_resident, const HostProgram &hp, int tail_n, int shape, const SpiceyKnobs &knobs) {
  std::vector<uint32_t> table;
  return u0_resident && shape >= 0 && shape < SPICEY_V2_NSHAPES && SPICEY_V2_SHAPES[shape].top_fold && !knobs.no_top_fold && hp.hdr.pcr_level >= 2 &&
         spicey_top_fold_table(hp, tail_n, table);
}
bool spicey_top_fold_run(const LaunchPlan &plan, int64_t steps) { return plan.top_fold && spicey_u0_resident_run(plan, steps); }

bool spicey_stamp_fuse_table(const HostProgram &hp, int tail_n, int T, int nsv, int nel, std::vector<uint32_t> &table) {
  table.clear();
  const SpiceyProg &P = hp.hdr;
  const bool linear = P.nD == 0 && P.nS == 0 && P.nDynEnt == 0;
  if (T <= 0 || nsv != 2 || nel != 2 || !P.has16 || P.hybrid || !P.fresh_fill || linear || P.nS != 0 || P.nL != 0 || !spicey_addr_fits(P, tail_n)) return false;
  // the beyond-capacity loops of B and Z (TranPhases2::set_remainders)
  if (P.nKeep > nsv * T || P.nDynEnt > nsv * T || P.nDynX > 0 || P.n > nel * T || P.nRowX > 0) return false;
  if (P.nOut > nel * T || P.nR > nel * T || P.nC > nel * T || P.nV > T || P.nD > nel * T) return false;
  if (hp.ent_dd.size() < (size_t)P.nKeep || hp.row_desc.size() < (size_t)P.n * 2) return false;
  if ((uint32_t)P.nKeep > 0x3FFFu || (uint32_t)(P.xoff + P.n) > 0x3FFFu) return false;
  const int oV = P.nC + P.nL, oD = P.nC + P.nL + P.nV;
  std::vector<uint32_t> ent((size_t)T * nsv, SPICEY_SF_NONE), row((size_t)T * nel, SPICEY_SF_NONE);  // [item][thread]
  std::vector<uint32_t> free_ent, free_row;
  for (int e = 0; e < P.nKeep; e++) {
    const uint32_t dd = hp.ent_dd[e];
    if (dd >> 31) return false;
    const uint32_t f[2] = {dd & 0x7fffu, (dd >> 15) & 0x7fffu};
    uint32_t w = (uint32_t)e | ((dd & (1u << 30)) ? SPICEY_SF_RECIP : 0u);
    int item = -1;
    for (int q = 0; q < 2; q++) {
      if (!f[q]) continue;
      const int i = (int)((f[q] & 0x3fffu) - 1u) - P.nS;
      if (i < 0 || i >= P.nD || (item >= 0 && item != i)) return false;
      item = i;
      w |= (q ? SPICEY_SF_F1 : SPICEY_SF_F0) | ((f[q] & 0x4000u) ? (q ? SPICEY_SF_F1_NEG : SPICEY_SF_F0_NEG) : 0u);
    }
    if (item < 0) { free_ent.push_back(w); continue; }
    uint32_t &slot = ent[(size_t)(item / T) * T + (size_t)(item % T)];
    if (slot != SPICEY_SF_NONE) return false;
    slot = w;
  }
  std::vector<uint32_t> src_row((size_t)P.nV, SPICEY_SF_NONE);
  for (int r = 0; r < P.n; r++) {
    const uint32_t d0 = hp.row_desc[(size_t)r * 2], d1 = hp.row_desc[(size_t)r * 2 + 1];
    if (d1 == 0xFFFFFFFFu) return false;
    const uint32_t f[4] = {d0 & 0xffffu, d0 >> 16, d1 & 0xffffu, d1 >> 16};
    uint32_t w = (uint32_t)(P.xoff + r);
    int item = -1, nfield = 0, source = -1;
    for (int q = 0; q < 4; q++) {
      if (!f[q]) continue;
      nfield++;
      const int ix = (int)((f[q] & 0x7fffu) - 1u);
      const bool neg = (f[q] & 0x8000u) != 0;
      int i;
      if (ix < P.nC) {  // gc v of capacitor ix
        i = ix;
        if (w & SPICEY_SF_F0) return false;
        w |= SPICEY_SF_F0 | (neg ? SPICEY_SF_F0_NEG : 0u);
      } else if (ix >= oD && ix < oD + P.nD) {  // ieq of diode ix - oD
        i = ix - oD;
        if (w & SPICEY_SF_F1) return false;
        w |= SPICEY_SF_F1 | (neg ? SPICEY_SF_F1_NEG : 0u) | ((w & SPICEY_SF_F0) ? 0u : SPICEY_SF_SWAP);
      } else if (ix >= oV && ix < oV + P.nV) {
        if (neg || source >= 0) return false;
        source = ix - oV;
        continue;
      } else {
        return false;
      }
      if (item >= 0 && item != i) return false;
      item = i;
    }
    if (source >= 0) {
      if (nfield != 1 || src_row[source] != SPICEY_SF_NONE) return false;
      src_row[source] = (uint32_t)(P.xoff + r);
      continue;
    }
    if (!(w & SPICEY_SF_F0)) w &= ~SPICEY_SF_SWAP;  // (a diode's field alone: there is no order to keep)
    if (item < 0) { free_row.push_back(w); continue; }
    uint32_t &slot = row[(size_t)(item / T) * T + (size_t)(item % T)];
    if (slot != SPICEY_SF_NONE) return false;
    slot = w;
  }
  for (int t = 0; t < P.nV; t++)
    if (src_row[t] == SPICEY_SF_NONE) return false;
  size_t at = 0;
  for (uint32_t w : free_ent) {
    while (at < ent.size() && ent[at] != SPICEY_SF_NONE) at++;
    if (at == ent.size()) return false;
    ent[at] = w;
  }
  at = 0;
  for (uint32_t w : free_row) {
    while (at < row.size() && row[at] != SPICEY_SF_NONE) at++;
    if (at == row.size()) return false;
    row[at] = w;
  }
  table.assign(spicey_stamp_fuse_words(T), SPICEY_SF_NONE);
  for (int t = 0; t < T; t++)
    for (int j = 0; j < 2; j++) {
      table[(size_t)t * SPICEY_STAMP_FUSE_THREAD_WORDS + j] = ent[(size_t)j * T + t];
      table[(size_t)t * SPICEY_STAMP_FUSE_THREAD_WORDS + 2 + j] = row[(size_t)j * T + t];
    }
  for (int t = 0; t < P.nV; t++) table[(size_t)t * SPICEY_STAMP_FUSE_THREAD_WORDS + 4] = src_row[t];
  return true;
}
bool spicey_plan_stamp_fuse(bool top_fold, const HostProgram &hp, int tail_n, int T, int shape, const SpiceyKnobs &knobs) {
  std::vector<uint32_t> table;
  return top_fold && shape >= 0 && shape < SPICEY_V2_NSHAPES && SPICEY_V2_SHAPES[shape].stamp_fuse && T == SPICEY_V2_SHAPES[shape].threads && !knobs.no_stamp_fuse &&
         spicey_stamp_fuse_table(hp, tail_n, T, SPICEY_V2_SHAPES[shape].nsv, SPICEY_V2_SHAPES[shape].nel, table);
}
bool spicey_stamp_fuse_run(const LaunchPlan &plan, int64_t steps) { return plan.stamp_fuse && spicey_top_fold_run(plan, steps); }

bool spicey_fixed_schedule_fits(const HostProgram &hp, const HostResident &hres) {
  const SpiceyProg &P = hp.hdr;
  const int nL = P.nLevels, nPh = (int)hp.ph_cnt.size(), S = spicey_top_stages(P.pcr_n);
  if (!P.has16 || P.hybrid || P.pcr_n <= 0 || P.pcr_n > 64 || S < 1 || S > 6 || P.pcr_level < 2 || P.pcr_level > nL || nPh != 2 * nL || nPh > 254) return false;
  if (hres.tail_n != 0 || hres.rmax <= 0 || hres.T <= 0 || (hres.T & 63)) return false;
  const int u_end = P.pcr_level, k_begin = 2 * nL - P.pcr_level;
  if (k_begin >= 2 * nL - 1 || hres.k_merge != k_begin) return false;  // (a merged backward phase and a last one behind it)
  if ((int)hres.st_cnt.size() < nPh || hres.st_cnt[0] == 0u) return false;
  for (int p = 1; p < nPh; p++)
    if (hres.st_cnt[p] != 0u) return false;
  for (int p = 0; p < u_end - 1; p++)
    if (hp.ph_cnt[p] == 0u) return false;  // (not unsafe, but a barrier per step for nothing: launch_plan.h)
  // the resident records: slot s of wave w runs in phase res_phase[w][s]; 0xFE = the continuation of the row record before it
  const int nW = hres.T / 64, rmax = hres.rmax;
  if (hres.res_phase.size() < (size_t)nW * rmax || hres.res.size() < (size_t)rmax * hres.T * 4) return false;
  for (int w = 0; w < nW; w++)
    for (int s = 0; s < rmax; s++) {
      const int ph = hres.res_phase[(size_t)w * rmax + s];
      if (ph < 0 || ph == 0xFE) continue;
      const bool factor = ph < nL;
      if (factor ? ph >= u_end - 1 : ph < k_begin) continue;  // (the folded level, the top's own levels: never dispatched)
      if (factor && s + 1 < rmax && hres.res_phase[(size_t)w * rmax + s + 1] == 0xFE) continue;  // (a row record: two pivots by its form)
      for (int lane = 0; lane < 64; lane++) {
        const uint32_t w0 = hres.res[((size_t)s * hres.T + (size_t)w * 64 + lane) * 4];
        if (((w0 >> 24) & SPICEY_R16_VALID) && ((w0 >> 16) & 0xffu) > 2u) return false;
      }
    }
  return true;
}
bool spicey_plan_fixed_schedule(bool stamp_fuse, const HostProgram &hp, const HostResident &hres, int shape, int debug_empty, const SpiceyKnobs &knobs) {
  return stamp_fuse && shape >= 0 && shape < SPICEY_V2_NSHAPES && SPICEY_V2_SHAPES[shape].fixed_schedule && hres.T == SPICEY_V2_SHAPES[shape].threads &&
         hres.rmax == SPICEY_V2_SHAPES[shape].rmax && debug_empty == 0 && !knobs.no_fixed_schedule && spicey_fixed_schedule_fits(hp, hres);
}
bool spicey_fixed_schedule_run(const LaunchPlan &plan, int64_t steps) { return plan.fixed_schedule && spicey_stamp_fuse_run(plan, steps); }

size_t spicey_zpar_doubles(const LaunchPlan &plan, const HostProgram &hp) {
  if (!plan.early || plan.interp != 2) return 0;
  const int shape = spicey_v2_shape(plan.T, plan.packed, hp.hdr.hybrid != 0, plan.packed && hp.hdr.fresh_fill != 0);
  if (shape < 0) return 0;
  return spicey_zpar_record_doubles(plan.n_inst, SPICEY_V2_SHAPES[shape].nel, plan.T);
}

void fill_info(const LaunchPlan &plan, const HostProgram &hp, const HostResident &hres, const SpiceyOptions &opt, SpiceyInfo *info) {
  const SpiceyProg &P = hp.hdr;
  memset(info, 0, sizeof(*info));
  info->n_var = P.n;
  if (plan.interp == 3) {  // reference-order engine: one workgroup per instance, no program; the rest does not apply
    info->threads = plan.T;
    info->inst_per_wg = 1;
    info->lds_bytes = plan.lds ? (int32_t)plan.lds_bytes : 0;
    info->n_cur = P.nCur;
    info->n_out = P.nOut;
    info->n_workgroups = plan.grid;
    info->interpreter = 3;
    info->wgs_per_inst = 1;
    return;
  }
  info->nnz_a = hp.nnzA;
  info->nnz_lu = P.nLU;
  info->n_levels = P.nLevels;
  info->threads = plan.T;
  info->inst_per_wg = plan.K;
  info->lds_bytes = plan.lds ? (int32_t)plan.lds_bytes : 0;
  info->n_cur = P.nCur;
  info->n_out = P.nOut;
  info->n_workgroups = plan.grid;
  info->interpreter = plan.interp;
  info->geometry = plan.interp == 2 ? (plan.packed ? 2 : 1) : 0;
  info->tail_levels = hres.tail_n;
  info->wgs_per_inst = plan.G;
  info->resident_slots = plan.interp == 2 ? hres.rmax : 0;
  info->resident_tasks = hres.resident_tasks;
  info->streamed_tasks = hres.streamed_tasks;
  info->program_bytes = (int64_t)hp.blob.size();
  info->algorithmic_bytes_solve = plan.algo_bytes;
  info->factor_reuse = (P.nD == 0 && P.nS == 0 && P.nDynEnt == 0 && !((opt.debug >> 1) & 1)) ? 1 : 0;
  info->n_fronts = P.nFronts;
  info->front_cut = P.front_cut;
  info->max_front = P.max_front_mp;
  info->front_ws_bytes = P.front_ws * (int64_t)sizeof(double);
  info->pcr_rows = (plan.interp == 2 && plan.K == 1) ? P.pcr_n : 0;
  info->pcr_level = info->pcr_rows ? P.pcr_level : 0;
  info->hybrid_entries = P.hybrid ? P.hyb_g0 + P.hyb_g2 : 0;
  info->operand_addr = (plan.interp == 2 && plan.addr) ? 1 : 0;
}
