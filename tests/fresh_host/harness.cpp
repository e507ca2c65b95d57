// tests/fresh_host/harness.cpp — CPU harness of the fresh-fill programs (TEST INFRASTRUCTURE ONLY).
//
// Compiles the emulator's sources unchanged (tests/emul/emul.cpp: the sequential executor, and with it symbolic.cpp,
// launch_plan.cpp and tran_exec.h) and adds what the fresh-fill tests need: the builder's invariants checked on the
// program as the device gets it, a run of the packed layout (512 threads, 4 slots) on the build a program belongs to —
// <4, 6, 2> for the default program, <4, 2, 2> for a fresh-fill one — with the workspace pre-filled with NaN on request,
// and the launch plan's choice between the two.
#include "../emul/emul.cpp"

#include <cmath>
#include <limits>

namespace {

// One factor target of a phase as either encoding states it: entry, flagged or not
struct Tgt { uint32_t e; bool fresh; };

// Targets and operand reads (entries only: indices below nLU) of `count` generic factor records from 16-byte unit `first`
void walk_generic(const HostProgram &hp, const std::vector<uint32_t> &arr, size_t first, size_t count, std::vector<Tgt> &tg, std::vector<uint32_t> &ops) {
  const uint32_t nLU = (uint32_t)hp.hdr.nLU;
  for (size_t i = 0; i < count; i++) {
    const uint32_t *w = &arr[(first + i) * 4];
    const uint32_t meta = w[0] >> 16, tgt = w[0] & 0xffffu, cnt = meta & 0xffu, flags = meta >> 8;
    if (!(flags & SPICEY_R16_VALID)) continue;
    if (tgt < nLU) tg.push_back({tgt, (flags & SPICEY_R16_FRESH) != 0});
    else if (flags & SPICEY_R16_FRESH) tg.push_back({tgt, true});  // (a flagged right-hand side: reported as outside the class)
    const bool rhs = tgt >= nLU;
    auto triple = [&](uint32_t l, uint32_t d, uint32_t u) {
      ops.push_back(l); ops.push_back(d);
      if (!rhs) ops.push_back(u);  // (a right-hand-side task's third operand is y_k)
    };
    if (cnt <= 2) {
      const uint32_t h[6] = {w[1] & 0xffffu, w[1] >> 16, w[2] & 0xffffu, w[2] >> 16, w[3] & 0xffffu, w[3] >> 16};
      for (uint32_t j = 0; j < cnt; j++) triple(h[3 * j], h[3 * j + 1], h[3 * j + 2]);
    } else {
      for (uint32_t j = 0; j < cnt; j++) triple(hp.ovf16[w[3] + 3 * j], hp.ovf16[w[3] + 3 * j + 1], hp.ovf16[w[3] + 3 * j + 2]);
    }
  }
}

void walk_rows(const HostProgram &hp, size_t first_unit, size_t rows, std::vector<Tgt> &tg, std::vector<uint32_t> &ops) {
  for (size_t i = 0; i < rows; i++) {
    const uint32_t *w = &hp.fus16[first_unit * 4 + i * 8];
    uint16_t h[16];
    for (int q = 0; q < 8; q++) { h[2 * q] = (uint16_t)(w[q] & 0xffffu); h[2 * q + 1] = (uint16_t)(w[q] >> 16); }
    const uint32_t meta = h[1];
    if (!((meta >> 8) & SPICEY_R16_VALID)) continue;
    tg.push_back({h[0], (meta & SPICEY_ROW_FRESH_AII) != 0});
    for (uint32_t p = 0; p < (meta & 3u); p++) {
      const uint16_t *q = h + 3 + 6 * p;
      ops.push_back(q[0]); ops.push_back(q[1]); ops.push_back(q[2]);
      if ((meta >> (4 + p)) & 1u) {
        ops.push_back(q[4]);
        tg.push_back({q[5], (meta & (p == 0 ? SPICEY_ROW_FRESH_O0 : SPICEY_ROW_FRESH_O1)) != 0});
      }
    }
  }
}

int32_t build(const SpiceyDesc *d, HostProgram &hp, int32_t pcr_top, int32_t fresh) {
  std::string err;
  return spicey_build_program(d, hp, err, true, 0, pcr_top != 0, false, fresh != 0);
}

}  // namespace

// The invariants of a program built with fresh_fill, from the sections the device reads.  out[0..3] = nKeep, nRestore, nLU,
// entries of the class; out[4..]: violations by kind —
//   [4] an entry of [nKeep, nRestore) with a static or a dynamic stamp
//   [5] an entry of the class that some record targets and whose flagged tasks are not exactly one (rec16 encoding)
//   [6] an entry of the class whose first targeting phase does not hold the flag, or a later one does
//   (an entry of the class that NO record targets is a fill among the pivots of a tridiagonal top, which cyclic reduction
//   never forms: it must be untouched — [11] counts those that a factor or backward record or the top's table reads, or
//   that exist in a program without a top; out[3] - untargeted = the entries the checks [5], [6] ran on)
//   [7] an operand read of an entry of the class in the phase that creates it or an earlier one (either encoding)
//   [8] a flag on a target outside the class (either encoding)
//   [9] a phase whose row-record encoding flags other entries than its generic one
//   [10] has16 (0: the program has no 16-bit records and the record checks did not run)
extern "C" int32_t spicey_fresh_check(const SpiceyDesc *d, int32_t pcr_top, int32_t fresh, int64_t *out /*[12]*/) {
  for (int i = 0; i < 12; i++) out[i] = 0;
  HostProgram hp;
  const int32_t rc = build(d, hp, pcr_top, fresh);
  if (rc != SPICEY_OK) return rc;
  const SpiceyProg &h = hp.hdr;
  const uint32_t nK = (uint32_t)h.nKeep, nR = (uint32_t)h.nRestore, nLU = (uint32_t)h.nLU;
  out[0] = nK; out[1] = nR; out[2] = nLU; out[3] = nR - nK; out[10] = h.has16;
  auto in_class = [&](uint32_t e) { return e >= nK && e < nR; };
  for (uint32_t e = nK; e < nR; e++)
    if (hp.stat_ptr[e + 1] != hp.stat_ptr[e] || (hp.ent_flag[e] & 2) || (hp.ent_dd[e] & 0xbfffffffu)) out[4]++;
  if (!h.has16) return SPICEY_OK;
  const int nL = h.nLevels;
  std::vector<int> first_phase(nLU, -1), flagged(nLU, 0), flagged_at(nLU, -1);
  std::vector<std::vector<uint32_t>> ops(nL), ops_rows(nL);
  for (int p = 0; p < nL; p++) {
    std::vector<Tgt> tg;
    walk_generic(hp, hp.rec16, hp.ph_first[p], hp.ph_cnt[p], tg, ops[p]);
    std::vector<uint32_t> fl;
    for (const Tgt &t : tg) {
      if (t.fresh && !(t.e < nLU && in_class(t.e))) { out[8]++; continue; }
      if (t.e >= nLU) continue;
      if (first_phase[t.e] < 0) first_phase[t.e] = p;
      if (t.fresh) { flagged[t.e]++; flagged_at[t.e] = p; fl.push_back(t.e); }
    }
    if (hp.fus_pairs[p] > 0) {  // the same phase as row records + generic remainder
      std::vector<Tgt> tr;
      walk_generic(hp, hp.fus16, hp.fus_first[p], hp.fus_gen[p], tr, ops_rows[p]);
      walk_rows(hp, (size_t)hp.fus_first[p] + hp.fus_gen[p], hp.fus_pairs[p], tr, ops_rows[p]);
      std::vector<uint32_t> fr;
      for (const Tgt &t : tr) {
        if (t.fresh && !(t.e < nLU && in_class(t.e))) { out[8]++; continue; }
        if (t.fresh) fr.push_back(t.e);
      }
      std::sort(fl.begin(), fl.end());
      std::sort(fr.begin(), fr.end());
      if (fl != fr) out[9]++;
    }
  }
  std::vector<char> read_by_any(nLU, 0);
  for (int p = 0; p < nL; p++)
    for (const std::vector<uint32_t> *o : {&ops[p], &ops_rows[p]})
      for (uint32_t e : *o) if (e < nLU) read_by_any[e] = 1;
  for (int p = nL; p < 2 * nL; p++)  // backward records: diagonal and U entries
    for (uint32_t i = 0; i < hp.ph_cnt[p]; i++) {
      const uint32_t *w = &hp.rec16[((size_t)hp.ph_first[p] + i) * 4];
      const uint32_t cnt = (w[0] >> 16) & 0xffu;
      read_by_any[w[1] & 0xffffu] = 1;
      if (cnt <= 2) { if (cnt >= 1) read_by_any[w[1] >> 16] = 1; if (cnt == 2) read_by_any[w[2] >> 16] = 1; }
      else for (uint32_t j = 0; j < cnt; j++) read_by_any[hp.ovf16[w[3] + 2 * j]] = 1;
    }
  for (uint16_t v : hp.pcr_tab) if (v != 0xFFFFu && v < nLU) read_by_any[v] = 1;
  for (uint32_t e = nK; e < nR; e++) {
    if (first_phase[e] < 0) {  // no task: only under a top, and then nothing may look at it
      out[11] += (h.pcr_n == 0 || read_by_any[e]) ? 1 : 0;
      out[3]--;
      continue;
    }
    if (flagged[e] != 1) out[5]++;
    if (flagged_at[e] != first_phase[e]) out[6]++;
  }
  for (int p = 0; p < nL; p++)
    for (const std::vector<uint32_t> *o : {&ops[p], &ops_rows[p]})
      for (uint32_t e : *o)
        if (e < nLU && in_class(e) && (first_phase[e] < 0 || first_phase[e] >= p)) out[7]++;
  return SPICEY_OK;
}

// One run at the packed layout (T threads, 4 slots) on the build the program belongs to; `flags` bit 0: threads of a
// phase in reverse order, bit 1: the workspace (entries, right-hand side, element vectors) starts as NaN.
// info6 = {nKeep, nRestore, streamed tasks, resident tasks, nDynEnt, fresh_fill of the program}.
extern "C" int32_t spicey_fresh_run(const SpiceyDesc *d, int32_t fresh, int32_t T, int64_t steps, double dt, const double *src, double *out_v, double *out_i,
                                    int32_t *iters, double *C_vprev, double *L_iprev, double *D_vdprev, int32_t *S_ison, int32_t flags, int64_t *info6) {
  HostProgram hp;
  int32_t rc = build(d, hp, 1, fresh);
  if (rc != SPICEY_OK) return rc;
  if (hp.structurally_singular || !hp.hdr.has16 || T <= 0 || (T & 63)) return SPICEY_ERR_BAD_DESC;
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
  HostResident hr;
  spicey_build_resident(hp, T, 4, hr, 24, true);
  SpiceyResident Q = hr.bind(hr.blob.data());
  if (info6) {
    info6[0] = P.nKeep; info6[1] = P.nRestore; info6[2] = hr.streamed_tasks; info6[3] = hr.resident_tasks; info6[4] = P.nDynEnt; info6[5] = P.fresh_fill;
  }
  const double fill = (flags & 2) ? std::numeric_limits<double>::quiet_NaN() : 0.0;
  for (int g = 0; g < ni; g++) {
    std::vector<double> W((size_t)P.nW, fill), u((size_t)P.nU + 1, fill), gd((size_t)P.nGdyn + 1, fill);
    std::vector<int32_t> ison((size_t)P.nS + 1), fl(4);
    std::vector<uint32_t> tail((size_t)(hr.tail_n + 6) * 64 * 4);
    WgCtx<1> c;
    c.W = W.data(); c.u = u.data(); c.gd = gd.data(); c.ison = ison.data(); c.flags = fl.data(); c.tail = tail.data(); c.G = nullptr;
    c.valid[0] = true; c.inst[0] = g;
    SeqExec ex{T, (flags & 1) != 0};
    if (P.fresh_fill) {
      std::vector<ResRegs<1, 4, 2, 2>> regs(T);
      ex.rr = &regs;
      spicey_tran_run_v2<1, 4, 2, 2>(ex, P, Q, R, c, g);
    } else {
      std::vector<ResRegs<1, 4, 6, 2>> regs(T);
      ex.rr = &regs;
      spicey_tran_run_v2<1, 4, 6, 2>(ex, P, Q, R, c, g);
    }
  }
  for (int g = 0; g < ni; g++)
    if (status[(size_t)g * 4]) return SPICEY_ERR_SINGULAR;
  return SPICEY_OK;
}

// spicey_create's plan on a device of `ncu` CUs (knobs from the environment, as there): out8 = {fresh, packed, threads, nKeep,
// nRestore, nDynEnt, fresh_fill of the program the plan kept, index of the v2 build it launches}; info as spicey_emul_plan fills it.
extern "C" int32_t spicey_fresh_plan(const SpiceyDesc *d, const SpiceyOptions *opt, int32_t ncu, SpiceyInfo *info, int64_t *out8) {
  const SpiceyOptions o = opt ? *opt : SpiceyOptions{};
  const PlanDevice dev{[ncu](int, int *n, std::string &) { *n = ncu; return (int32_t)SPICEY_OK; }, [](const SpiceyProg &, int, int) { return 1; }};
  HostProgram hp;
  HostResident hres;
  LaunchPlan plan;
  std::string msg;
  const int32_t rc = spicey_plan(d, o, spicey_read_knobs(), dev, hp, hres, plan, msg);
  if (rc != SPICEY_OK) return rc;
  if (info) fill_info(plan, hp, hres, o, info);
  out8[0] = plan.fresh; out8[1] = plan.packed; out8[2] = plan.T; out8[3] = hp.hdr.nKeep; out8[4] = hp.hdr.nRestore; out8[5] = hp.hdr.nDynEnt;
  out8[6] = hp.hdr.fresh_fill;
  out8[7] = plan.interp == 2 ? spicey_v2_shape(plan.T, plan.packed, hp.hdr.hybrid != 0, plan.packed && hp.hdr.fresh_fill != 0) : -1;
  return SPICEY_OK;
}
