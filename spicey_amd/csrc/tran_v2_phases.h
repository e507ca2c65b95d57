// tran_v2_phases.h — the v2 B / S / Z phases, TranPhases2 (tran_exec.h is the map).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "program.h"
#include "tran_common.h"
#include "tran_pt.h"
#include "tran_rec16.h"
#include "tran_v1_phases.h"

// v2 versions of the B and Z phases: everything step-invariant that a thread needs (static entry values,
// stamp / right-hand-side descriptors, element terminals, vPrev) sits in its registers; items beyond the
// resident capacity (entries >= NSV*T, rows / elements >= T) take the streamed remainder loops.
// Difference to v1: u[c] holds the capacitor companion CURRENT gc*vPrev (so the right-hand side is a
// pure +-1 gather, stampCurrentReal.ts:12-13) and the exact vPrev lives in a register.
// HYB: the hybrid workspace layout (program.h, SpiceyProg::hybrid) — entry ids below hyb_g0 and in [nRestore, nRestore + hyb_g2)
// are leaf-owned and live in the global array c.G, all others in LDS at id - hyb_g0 (- hyb_g2 above nRestore); the
// right-hand side starts at LDS index P.xoff; c.u / c.gd point to global memory.
// EP: the early-prefetch build (K = 1, LDS workspace) — Z's element parameters come from the per-thread record SpiceyRun::zpar
// and are fetched, with the next step's source value, between the factor and the backward phases instead of at the tail of
// the last backward one; B then fetches and parks nothing (spicey_tran_run_v2 places the calls: see there for where).  A compile-time property of a build, like
// FRESH: a kernel that holds both forms of B and Z does not fit the 128 registers of the packed builds.
// OS: the operand-slot build (an early-prefetch build with the phase table, tran_pt_layout.h: spicey_slot_index) — two read-only
// constants in LDS take the place of conditions that were evaluated again in every step.  Z: the terminal indices that
// load_resident keeps in registers name the +0.0 slot where the netlist says ground, so the resident section reads
// c.W[index] and subtracts, with no compare and no select (14 index halves per thread and step: 56 vector instructions of
// Z's ~275); its eight result stores take a 32-bit lane offset on a wave-uniform section base, and the row bases come
// from the phase table with the instance's share already multiplied out (spicey_pt_rebase_rows).  B: an empty field of
// a resident stamp or right-hand-side descriptor names the -0.0 slot, so all operands of a thread's entries and rows are
// read together, one LDS round trip instead of six dependent ones (dd_slots / rhs_slots below).  Everything that
// decodes a descriptor from global memory (the beyond-capacity loops of B and Z, a_reiterate, z_lin_err) is unchanged.
// RA: the ready-argument build (an operand-slot build) — Z's head moves to scalars only what its always-executed code
// reads (spicey_pt_args_z); the end-state arrays of the last step, and the record and the source table where nothing was
// prefetched, are read from the table inside their own branch (`ptab`); the record and the source table are this instance's
// already (spicey_pt_rebase_ready), so the early fetch loads with a scalar base and a 32-bit lane offset; the per-step
// offsets step x row are one 32 x 32 -> 64-bit product (tran_pt_layout.h: spicey_ready_steps_ok).  Same values from the same
// addresses in the same order as the OS build.
// OA: the operand-address build (a ready-argument build; tran_common.h: SpiceyOperand) — c.W is LDS address 0, and the
// always-executed reads of Z's resident section name their operands by handles made of the terminal words' halves in one
// instruction.  B's resident descriptors are re-encoded once more in the prologue (dd_addr / rhs_addr below): their fields
// index c.gd and c.u, which lie behind W in the same array, and become indices from the start of W, so that no scalar
// base stands in their addresses either; spicey_addr_fits has made sure that the fields hold the largest of them, the
// -0.0 slot.  Same operands, same order, same arithmetic as the RA build.
// SF: the stamp fuse (an operand-address build; tran_v2_run.h has where the phases stand) — Z is two phases.  The first is Z
// as it stands, but its capacitors and diodes write nothing to LDS: it forms the next step's stamped entries and
// right-hand-side rows from the thread's OWN conductances and companion currents, in the order of the descriptor's fields,
// writes the entries straight into W and keeps the rows; the second (z_fuse), behind a barrier, writes the rows over the
// solution.  The descriptor registers hold the slot words of the host's table (launch_plan.h: spicey_stamp_fuse_table;
// sf_load), and what crosses the barrier between the two phases rides in registers that are dead there: pf[j][0] = row
// slot j's sum, srcn = the row of the thread's source.  c.gd and c.u are not written in the time loop.
template <int K, int RMAX, int NSV, int NEL, bool HYB = false, bool EP = false, bool OS = false, bool RA = false, bool OA = false, bool SF = false>
struct TranPhases2 {
  static_assert(!SF || (OA && NSV == 2 && NEL == 2 && ResRegs<K, RMAX, NSV, NEL>::NDD == 2), "the stamp fuse is built into the operand-address kernel of the fresh packed shape");
  static_assert(!EP || (K == 1 && !HYB), "the early prefetch is built for one instance per workgroup on the LDS workspace");
  static_assert(!OS || EP, "the operand slots are built into the early-prefetch kernels");
  static_assert(!RA || OS, "the ready arguments are built into the operand-slot kernels");
  static_assert(!OA || (RA && K == 1 && !HYB), "the operand addresses are built into the ready-argument kernels: one instance per workgroup, LDS workspace");
  typedef SpiceyOperand<OA> Op;
  const SpiceyProg &P;
  const SpiceyRun &R;
  WgCtx<K> &c;
  int T;
  // where entry `e` (an id below nRestore: what phase B re-stamps) is stored
  SPICEY_HD void put_entry(uint32_t e, int k, double v) const {
    if (HYB) {
      if (e < (uint32_t)P.hyb_g0) c.G[(size_t)e * K + k] = v;
      else c.W[(size_t)(e - (uint32_t)P.hyb_g0) * K + k] = v;
    } else {
      c.W[(size_t)e * K + k] = v;
    }
  }
  // Which of the beyond-resident-capacity loops of B / Z have any work (wave-uniform, fixed for the run).  On the
  // circuits the resident geometry is sized for they are all empty, yet each one costs a bound fetch, address
  // arithmetic and a branch: ~1200 cycles per step in Z alone before they were put behind one test.
  uint32_t brem, zrem;
  // With the phase table, P and R above are LOCAL structs that hold only the fields the always-executed code of B, Z and
  // the parameter prefetch reads (spicey_pt_args), and Pg / Rg point to the complete argument structs in global memory:
  // the beyond-resident-capacity loops and the diagnostics, which read many more fields on few circuits, take a fresh copy
  // from there inside their own branch (SPICEY_COLD_ARGS).  Null: P and R are complete.
  const SpiceyProg *Pg = nullptr;
  const SpiceyRun *Rg = nullptr;
  // fresh build, for u0_fetch: the phase table (null: none — then Qg, the resident struct where it lives, says where phase
  // 0's records are); RA: Z's and the early fetch's lazy reads go there too
  const uint32_t *ptab = nullptr;
  const SpiceyResident *Qg = nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
#define SPICEY_COLD_STRUCT(whole, here) ((whole) ? spicey_fresh(*(whole)) : (here))
#else
#define SPICEY_COLD_STRUCT(whole, here) ((whole) ? *(whole) : (here))
#endif
#define SPICEY_COLD_ARGS                                             \
  const SpiceyProg &P = SPICEY_COLD_STRUCT(this->Pg, this->P); \
  const SpiceyRun &R = SPICEY_COLD_STRUCT(this->Rg, this->R);  \
  (void)P;                                                           \
  (void)R
  typedef ResRegs<K, RMAX, NSV, NEL> Regs;
  // the diagnostics of SpiceyOptions.diagnostics are compiled into every geometry but the two-workgroups-per-CU one (NSV = 6:
  // 128 VGPRs and nothing to spare — with them that kernel spills, which the build refuses); the host keeps a handle with
  // the option out of that geometry
  static constexpr bool DIAG = !SpiceyShapeKind<RMAX, NSV, NEL>::packed && !HYB;  // (nor into the hybrid-workspace build, for the same reason)
  // fresh-fill build: B, and the copy that fills the registers it restores from, stop at the kept targets — the fresh class
  // [nKeep, nRestore) is created by its flagged factor tasks in every solve and nothing reads it before them
  static constexpr bool FRESH = SpiceyShapeKind<RMAX, NSV, NEL>::fresh;
  SPICEY_HD int n_stamped() const { return FRESH ? P.nKeep : P.nRestore; }
  // hybrid builds: items of a beyond-resident loop whose loads are in flight together (the 1024-thread build has 128 registers)
  static constexpr int BW = NEL >= 2 ? 4 : 2;   // (phase Z)
  static constexpr int BWB = BW;                 // (phase B; four at a time in the 1024-thread build compiled — 126 registers — and was 5 % slower per step)
  SPICEY_HD void set_remainders() {
    brem = (n_stamped() > NSV * T ? 1u : 0u) | (P.nDynX > 0 ? 2u : 0u) | (P.n > NEL * T ? 4u : 0u) | (P.nRowX > 0 ? 8u : 0u) |
           (P.nDynEnt > Regs::NDD * T ? 16u : 0u);
    zrem = (P.nOut > NEL * T ? 1u : 0u) | (P.nR > NEL * T ? 2u : 0u) | (P.nC > NEL * T ? 4u : 0u) | (P.nL > 0 ? 8u : 0u) |
           (P.nV > T ? 16u : 0u) | (P.nS > 0 ? 32u : 0u) | (P.nD > NEL * T ? 64u : 0u);
    brem = (uint32_t)SPICEY_UNIFORM((int)brem);
    zrem = (uint32_t)SPICEY_UNIFORM((int)zrem);
  }

  // branch-free: ground (0xFFFF) reads slot 0, a valid address, and is masked afterwards, so that the reads of
  // several elements can be issued back to back instead of one exec-masked block each
  SPICEY_HD double volt16(uint32_t xi, int k) const {
    const double v = c.W[(size_t)(xi == 0xFFFFu ? 0u : xi) * K + k];
    return xi == 0xFFFFu ? 0.0 : v;
  }
  SPICEY_HD double dv16(uint32_t ab, int k) const { return volt16(ab & 0xFFFFu, k) - volt16(ab >> 16, k); }

  // OS: a register-resident index (one 16-bit half; ground already names the +0.0 slot) and a pair of them
  // (through the half's handle: in an OA build one instruction from the word to the LDS address)
  template <int H>
  SPICEY_HD double volt_res(uint32_t ab) const { return Op::template ld<1>(c.W, Op::template half<H>(ab), 0); }
  SPICEY_HD double dv_res(uint32_t ab) const { return volt_res<0>(ab) - volt_res<1>(ab); }
  static SPICEY_HD uint32_t slot_pair(uint32_t ab, uint32_t zs) {
    const uint32_t a = ab & 0xFFFFu, b = ab >> 16;
    return (a == 0xFFFFu ? zs : a) | ((b == 0xFFFFu ? zs : b) << 16);
  }

  // OS, phase B: the descriptors of the resident entries and rows name an operand in EVERY field — a field that the program
  // leaves empty reads the -0.0 slot with the add sign (x + (-0.0) == x, bit for bit, for every x), so all conductances of a
  // thread's entries and all contributions of its rows are read unconditionally and together, then combined in the
  // order of stamp_entry / rhs_row.  Same registers, other fields:
  //   dd     bits 0-13 / 15-28: index into c.gd (no + 1), bit 14 / 29: subtract; bit 30: reciprocal; bit 31: not mine to stamp
  //   rhs[2] four 16-bit fields: bits 0-13 index into c.u (no + 1), bit 15: subtract; bit 14 of the LAST field: not a resident row
  // zg / zu: the -0.0 slot as an index into c.gd / c.u; spicey_slots_fit has made sure that 14 bits hold them.
  static SPICEY_HD uint32_t dd_slots(uint32_t dd, uint32_t zg) {
    const bool mine = !(dd >> 31);
    const uint32_t f0 = mine ? dd & 0x7fffu : 0u, f1 = mine ? (dd >> 15) & 0x7fffu : 0u;
    const uint32_t g0 = f0 ? (((f0 & 0x3fffu) - 1u) | (f0 & 0x4000u)) : zg, g1 = f1 ? (((f1 & 0x3fffu) - 1u) | (f1 & 0x4000u)) : zg;
    return g0 | (g1 << 15) | (dd & 0xC0000000u);
  }
  static SPICEY_HD void rhs_slots(uint32_t &d0, uint32_t &d1, uint32_t zu) {
    const bool mine = d1 != 0xFFFFFFFFu;
    uint32_t g[4];
    const uint32_t f[4] = {d0 & 0xffffu, d0 >> 16, d1 & 0xffffu, d1 >> 16};
    for (int i = 0; i < 4; i++) g[i] = (mine && f[i]) ? (((f[i] & 0x7fffu) - 1u) | (f[i] & 0x8000u)) : zu;
    d0 = g[0] | (g[1] << 16);
    d1 = g[2] | (g[3] << 16) | (mine ? 0u : 0x40000000u);
  }
  // OA, behind the two above: every field of a resident descriptor names an operand by now, and each index moves from the
  // start of c.gd / c.u to the start of W — `base` = nW + nU for dd, nW for rhs — in all fields at once (no carry leaves a
  // field: spicey_addr_fits).  Flags and signs stay where they are.
  static SPICEY_HD uint32_t dd_addr(uint32_t dd, uint32_t base) { return dd + base * ((1u << 15) | 1u); }
  static SPICEY_HD void rhs_addr(uint32_t &d0, uint32_t &d1, uint32_t base) { d0 += base * 0x10001u; d1 += base * 0x10001u; }
  // g, or -g where bit 31 of `flip` is set (every other bit of it is ignored): x + this is x + g or, bit for bit, x - g
  static SPICEY_HD double signed_by(double g, uint32_t flip) {
    uint64_t b;
    __builtin_memcpy(&b, &g, 8);
    b ^= (uint64_t)(flip & 0x80000000u) << 32;
    __builtin_memcpy(&g, &b, 8);
    return g;
  }

  // UR (the resident-record form of the fresh build, tran_v2_run.h): row record `tid` of factor phase 0 is loaded here, once
  // per run, from the address u0_fetch reads in every step of the other forms; a thread at or beyond the record count gets
  // zeros — no VALID flag, nothing executes.  (The host has made sure that the phase is streamed as row records, at most
  // one per thread and nothing else: spicey_plan_u0_resident.)
  template <bool UR = false>
  SPICEY_HD void load_resident(int tid, const SpiceyResident &Q, Regs &rr) const {
    if constexpr (UR) {
      static_assert(FRESH, "the resident level-0 record is a form of the fresh build");
      const uint32_t *dsc = Q.st_desc;  // (phase 0's descriptor: row-record flag, first record, count)
      const bool have = dsc[0] != 0u && (uint32_t)tid < dsc[2];
      for (int i = 0; i < 8; i++) rr.u0[FRESH ? i : 0] = 0u;
      if (have) {
        const uint32_t *src = P.fus16 + (size_t)dsc[1] * 4 + (size_t)tid * 8;
        for (int i = 0; i < 8; i++) rr.u0[FRESH ? i : 0] = src[i];
      }
    }
    for (int s = 0; s < RMAX; s++) {
      const bool have = s < Q.rmax;
      const uint32_t *src = Q.res + ((size_t)(have ? s : 0) * T + tid) * 4;
      rr.w0[s] = have ? src[0] : 0u; rr.w1[s] = have ? src[1] : 0u; rr.w2[s] = have ? src[2] : 0u; rr.w3[s] = have ? src[3] : 0u;
    }
    for (int s4 = 0; s4 < (RMAX + 3) / 4; s4++) {
      uint32_t pk = 0;
      for (int b = 0; b < 4; b++) {
        const int s = s4 * 4 + b;
        const int ph = s < Q.rmax && s < RMAX ? Q.res_phase[(size_t)(tid >> 6) * Q.rmax + s] : -1;
        pk |= (uint32_t)(ph < 0 ? 0xff : (ph & 0xff)) << (8 * b);
      }
      rr.phv[s4] = SPICEY_UNIFORM((int)pk);
    }
    rr.cursor = 0;
    for (int j = 0; j < NEL; j++) {
      const int i = tid + j * T;
      rr.rhs[j][0] = i < P.n ? P.row_desc[(size_t)i * 2] : 0u;
      rr.rhs[j][1] = i < P.n ? P.row_desc[(size_t)i * 2 + 1] : 0xFFFFFFFFu;  // 0xFFFFFFFF = not a resident row
      rr.eR[j] = i < P.nR ? P.R_ab[i] : 0xFFFFFFFFu;
      rr.eC[j] = i < P.nC ? P.C_ab[i] : 0xFFFFFFFFu;
      rr.eD[j] = i < P.nD ? P.D_ab[i] : 0xFFFFFFFFu;
      rr.ox[j] = i < P.nOut ? (P.out_x[i] < 0 ? 0xFFFFu : (uint32_t)P.out_x[i]) : 0xFFFFu;
    }
    if (OS) {  // ground, and an item that does not exist, read the +0.0 slot; the two constants are written here, once per run
      const uint32_t zs = spicey_slot_index(P);
      for (int j = 0; j < NEL; j++) {
        rr.eR[j] = slot_pair(rr.eR[j], zs); rr.eC[j] = slot_pair(rr.eC[j], zs); rr.eD[j] = slot_pair(rr.eD[j], zs);
        rr.ox[j] = rr.ox[j] == 0xFFFFu ? zs : rr.ox[j];  // (the upper half is still empty here)
        rhs_slots(rr.rhs[j][0], rr.rhs[j][1], zs + 1u - (uint32_t)P.nW);
        if (OA) rhs_addr(rr.rhs[j][0], rr.rhs[j][1], (uint32_t)P.nW);
      }
      if (tid == 0) { c.W[(size_t)zs] = 0.0; c.W[(size_t)zs + 1] = -0.0; }
    }
    if (tid < P.nV) rr.ox[0] |= (uint32_t)P.V_x[tid] << 16;  // upper half of ox[0]: W index of the branch current of source tid
  }
  // after p1_static: static entry values into registers; elements from the state entering the run
  SPICEY_HD void a0_initial(int tid, Regs &rr) const {
    const int oL = P.nC, oV = P.nC + P.nL, oD = P.nC + P.nL + P.nV;
    for (int j = 0; j < NSV; j++) {
      const int e = tid + j * T;
      if (j < Regs::NDD) rr.dd[j] = e < n_stamped() ? P.ent_dd[e] : 0x80000000u;  // bit 31 = "not mine to stamp"
      if (OS && j < Regs::NDD) rr.dd[j] = dd_slots(rr.dd[j], spicey_slot_index(P) + 1u - (uint32_t)(P.nW + P.nU));
      if (OA && j < Regs::NDD) rr.dd[j] = dd_addr(rr.dd[j], (uint32_t)(P.nW + P.nU));
      for (int k = 0; k < K; k++) rr.sv[j][k] = e < n_stamped() ? R.statv[(size_t)c.inst[k] * P.nLU + e] : 0.0;
    }
    for (int k = 0; k < K; k++) {  // entries that no phase ever writes: stamped once per run
      const double *sv = R.statv + (size_t)c.inst[k] * P.nLU;
      SPICEY_NOUNROLL
      for (int e = P.nRestore + tid; e < P.nLU; e += T) {
        if (HYB) {
          if (e < P.nRestore + P.hyb_g2) c.G[(size_t)e * K + k] = sv[e];  // leaf-owned: read from the global array by phase U_0 / K_0
          else c.W[(size_t)(e - P.hyb_g0 - P.hyb_g2) * K + k] = sv[e];
        } else {
          c.W[(size_t)e * K + k] = sv[e];
        }
      }
    }
    for (int k = 0; k < K; k++) {
      const size_t in = (size_t)c.inst[k];
      const double *g = R.gstat + in * P.nGstat;
      for (int j = 0; j < NEL; j++) rr.vprev[j][k] = tid + j * T < P.nC ? R.C_vprev[in * P.nC + tid + j * T] : 0.0;
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nC; i += T) c.u[(size_t)i * K + k] = g[P.nR + i] * R.C_vprev[in * P.nC + i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nL; i += T) c.u[(size_t)(oL + i) * K + k] = R.L_iprev[in * P.nL + i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nV; i += T) c.u[(size_t)(oV + i) * K + k] = R.src[in * R.src_stride + i];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nS; i += T) {
        const int on = R.S_ison[in * P.nS + i];
        c.ison[(size_t)i * K + k] = on;
        c.gd[(size_t)i * K + k] = spicey_switch_g(on, R.S_ron[in * P.nS + i], R.S_roff[in * P.nS + i]);
      }
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nD; i += T) {
        const double *dp = R.dpar + (in * P.nD + i) * 2;
        double g2, q, irec;
        spicey_diode_k<FRESH>(R.D_vdprev[in * P.nD + i], R.D_is[in * P.nD + i], dp[0], dp[1], false, g2, q, irec);
        c.gd[(size_t)(P.nS + i) * K + k] = g2;
        c.u[(size_t)(oD + i) * K + k] = q;
        if (DIAG && R.lin_vd && c.valid[k]) R.lin_vd[in * P.nD + i] = R.D_vdprev[in * P.nD + i];
      }
    }
    if (tid == 0) c.flags[0] = 0;
  }

  SPICEY_HD void stamp_entry(uint32_t e, uint32_t dd, const double *sv) const {  // sv[K]
    double v[K];
    for (int k = 0; k < K; k++) v[k] = sv[k];
    const uint32_t f0 = dd & 0x7fffu, f1 = (dd >> 15) & 0x7fffu;
    if (f0) {
      const uint32_t ix = (f0 & 0x3fffu) - 1;
      for (int k = 0; k < K; k++) { const double g = c.gd[(size_t)ix * K + k]; v[k] = (f0 & 0x4000u) ? v[k] - g : v[k] + g; }
    }
    if (f1) {
      const uint32_t ix = (f1 & 0x3fffu) - 1;
      for (int k = 0; k < K; k++) { const double g = c.gd[(size_t)ix * K + k]; v[k] = (f1 & 0x4000u) ? v[k] - g : v[k] + g; }
    }
    if (dd & (1u << 30))
      for (int k = 0; k < K; k++) {
        if (fabs(v[k]) < SPICEY_EPS && c.valid[k]) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
        v[k] = spicey_rcp(v[k]);
      }
    for (int k = 0; k < K; k++) put_entry(e, k, v[k]);
  }
  SPICEY_HD void rhs_row(uint32_t r, uint32_t d0, uint32_t d1) const {
    double acc[K];
    for (int k = 0; k < K; k++) acc[k] = 0.0;
    const uint32_t f[4] = {d0 & 0xffffu, d0 >> 16, d1 & 0xffffu, d1 >> 16};
    for (int i = 0; i < 4; i++)
      if (f[i]) {
        const uint32_t ix = (f[i] & 0x7fffu) - 1;
        for (int k = 0; k < K; k++) { const double t = c.u[(size_t)ix * K + k]; acc[k] = (f[i] & 0x8000u) ? acc[k] - t : acc[k] + t; }
      }
    for (int k = 0; k < K; k++) c.W[(size_t)(P.xoff + r) * K + k] = acc[k];
  }

  // ---- B: matrix = static + dynamic stamps; right-hand side -----------------------------------------
  SPICEY_HD void b_stamp(int tid, Regs &rr, bool reuse = false) const {
    SPICEY_MARK(c, 15);
    if (tid == 0) c.flags[0] = 0;
    rr.cursor = 0;  // a new solve walks the resident slots from the start
    if (!reuse) stamp_matrix(tid, rr);  // a linear circuit keeps the factors of step 0 in W
    rhs_rows(tid, rr);
  }
  // the whole of phase B: the next step's source values ride on it (a long phase with few live registers): fetched first,
  // parked in LDS last; Z moves them into place
  // Fresh build: factor phase 0 is the one phase of the packed chains that is still streamed, and the fetch of its first
  // record used to be an exposed L2 round trip at its head.  The record (row record `tid` of the phase: 32 bytes) is
  // loaded here instead, next to the source fetch, and has the whole of B to arrive.  Lanes without a record, and a phase
  // 0 that is resident or streams generic records, fetch nothing.
  SPICEY_HD void u0_fetch(int tid, Regs &rr) const {
    uint32_t rows, first, cnt;
    const uint32_t *fus16;
    if (ptab) {
      const SpiceyPtLanes d = SpiceyPtLanes::row(ptab, tid, 0);  // (row 0 = factor phase 0; the whole wave is here)
      rows = d.u32(0); first = d.u32(1); cnt = d.u32(2);
      fus16 = d.template ptr<const uint32_t>(SPICEY_PT_FUS16);
    } else {
      const uint32_t *dsc = spicey_fresh(*Qg).st_desc;
      rows = dsc[0]; first = dsc[1]; cnt = dsc[2];
      fus16 = P.fus16;
    }
    const bool have = rows != 0u && (uint32_t)tid < cnt;
    for (int i = 0; i < 8; i++) rr.u0[FRESH ? i : 0] = 0u;
    if (have) {
      const uint32_t *src = fus16 + (size_t)first * 4 + (size_t)tid * 8;
      for (int i = 0; i < 8; i++) rr.u0[FRESH ? i : 0] = src[i];
    }
  }
  // UR: the record is resident (load_resident) — B fetches nothing
  template <bool UR = false>
  SPICEY_HD void b_phase(int tid, int64_t step, Regs &rr, bool reuse) const {
    double sn = (K == 1 && !EP) ? z_src_fetch(tid, step, (size_t)c.inst[0]) : 0.0;  // (EP: fetched by z_early, parked by the last backward phase)
    if (FRESH && !UR) u0_fetch(tid, rr);
    SPICEY_SCHED_FENCE;
    b_stamp(tid, rr, reuse);
    SPICEY_SCHED_FENCE;
    if (K == 1 && !EP) z_src_park(tid, sn);
  }
  // ---- batched forms of the beyond-resident-capacity loops (HYB builds, K = 1) -------------------------------------------
  // Hybrid workspace: circuits of several thousand unknowns on 512 threads — most entries lie beyond the resident slots, and
  // one at a time each of them costs two or three DEPENDENT round trips to L2 (descriptor, static value, conductances).
  // Four at a time, every load of a stage issued before the first is used (the registers are there: this build is not at
  // the 128-register cap).  Same arithmetic per entry as stamp_entry.
  SPICEY_HD void stamp_rest_batched(int tid) const {
    const double *sv0 = R.statv + (size_t)c.inst[0] * P.nLU;
    // dynamic entries beyond the descriptor slots: [NDD T, nDynEnt)
    if (brem & 16u)
    SPICEY_NOUNROLL
    for (int e0 = tid + Regs::NDD * T; e0 < P.nDynEnt; e0 += BWB * T) {
      uint32_t dd[BWB];
      double v[BWB], ga[BWB], gb[BWB];
      SPICEY_UNROLL
      for (int b = 0; b < BWB; b++) {
        const int e = e0 + b * T;
        const bool have = e < P.nDynEnt;
        dd[b] = have ? P.ent_dd[e] : 0x80000000u;
        v[b] = sv0[have ? e : e0];
      }
      SPICEY_UNROLL
      for (int b = 0; b < BWB; b++) {
        const uint32_t f0 = dd[b] & 0x7fffu, f1 = (dd[b] >> 15) & 0x7fffu;
        const bool on = !(dd[b] >> 31);
        ga[b] = c.gd[(on && f0) ? (f0 & 0x3fffu) - 1 : 0u];
        gb[b] = c.gd[(on && f1) ? (f1 & 0x3fffu) - 1 : 0u];
      }
      SPICEY_UNROLL
      for (int b = 0; b < BWB; b++) {
        if (dd[b] >> 31) continue;
        const uint32_t f0 = dd[b] & 0x7fffu, f1 = (dd[b] >> 15) & 0x7fffu;
        double x = v[b];
        if (f0) x = (f0 & 0x4000u) ? x - ga[b] : x + ga[b];
        if (f1) x = (f1 & 0x4000u) ? x - gb[b] : x + gb[b];
        if (dd[b] & (1u << 30)) {
          if (fabs(x) < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
          x = spicey_rcp(x);
        }
        put_entry((uint32_t)(e0 + b * T), 0, x);
      }
    }
    // static update targets beyond the resident slots: plain copies of their static value, [max(NSV T, nDynEnt), nRestore)
    if (brem & 1u) {
      int e0 = tid + NSV * T;
      if (e0 < P.nDynEnt) e0 += ((P.nDynEnt - e0 + T - 1) / T) * T;
      SPICEY_NOUNROLL
      for (; e0 < P.nRestore; e0 += BWB * T) {
        double v[BWB];
        SPICEY_UNROLL
        for (int b = 0; b < BWB; b++) v[b] = sv0[e0 + b * T < P.nRestore ? e0 + b * T : e0];
        SPICEY_UNROLL
        for (int b = 0; b < BWB; b++)
          if (e0 + b * T < P.nRestore) put_entry((uint32_t)(e0 + b * T), 0, v[b]);
      }
    }
    if (brem & 2u)
    SPICEY_NOUNROLL
    for (int t = tid; t < P.nDynX; t += T) {  // entries with > 2 dynamic stamps (rare: kept one at a time)
      const uint32_t et = P.dynx_ent[t], e = SPICEY_IDX(et);
      double x = sv0[e];
      for (uint32_t j = P.dynx_ptr[t]; j < P.dynx_ptr[t + 1]; j++) {
        const uint32_t ix = P.dynx_idx[j];
        const double g = c.gd[SPICEY_IDX(ix)];
        x = (ix & SPICEY_NEG) ? x - g : x + g;
      }
      if (et & SPICEY_TGT_RECIP) {
        if (fabs(x) < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
        x = spicey_rcp(x);
      }
      put_entry(e, 0, x);
    }
  }
  // right-hand-side rows beyond the resident ones, four at a time: descriptors, then all their (up to 16) contributions
  SPICEY_HD void rhs_rest_batched(int tid) const {
    SPICEY_NOUNROLL
    for (int r0 = tid + NEL * T; r0 < P.n; r0 += BWB * T) {
      uint32_t d[BWB][2];
      double t[BWB][4];
      SPICEY_UNROLL
      for (int b = 0; b < BWB; b++) {
        const int r = r0 + b * T < P.n ? r0 + b * T : r0;
        d[b][0] = P.row_desc[(size_t)r * 2]; d[b][1] = P.row_desc[(size_t)r * 2 + 1];
        if (r0 + b * T >= P.n) d[b][1] = 0xFFFFFFFFu;
      }
      SPICEY_UNROLL
      for (int b = 0; b < BWB; b++) {
        const bool on = d[b][1] != 0xFFFFFFFFu;
        const uint32_t f[4] = {d[b][0] & 0xffffu, d[b][0] >> 16, d[b][1] & 0xffffu, d[b][1] >> 16};
        SPICEY_UNROLL
        for (int i = 0; i < 4; i++) t[b][i] = c.u[(on && f[i]) ? (f[i] & 0x7fffu) - 1 : 0u];
      }
      SPICEY_UNROLL
      for (int b = 0; b < BWB; b++) {
        if (d[b][1] == 0xFFFFFFFFu) continue;
        const uint32_t f[4] = {d[b][0] & 0xffffu, d[b][0] >> 16, d[b][1] & 0xffffu, d[b][1] >> 16};
        double acc = 0.0;
        SPICEY_UNROLL
        for (int i = 0; i < 4; i++)
          if (f[i]) acc = (f[i] & 0x8000u) ? acc - t[b][i] : acc + t[b][i];
        c.W[(size_t)(P.xoff + r0 + b * T)] = acc;
      }
    }
  }

  SPICEY_HD void stamp_matrix(int tid, Regs &rr) const {
    if (HYB) {
      // hybrid workspace: the conductances live in global memory — those of all descriptor slots are fetched together (one
      // L2 round trip) before the first entry is formed; then the plain restores; then the batched rest
      double ga[Regs::NDD], gb[Regs::NDD];
      SPICEY_UNROLL
      for (int j = 0; j < Regs::NDD; j++) {
        uint32_t dd = rr.dd[j];
        SPICEY_OPAQUE(dd);
        const uint32_t f0 = dd & 0x7fffu, f1 = (dd >> 15) & 0x7fffu;
        const bool on = !(dd >> 31);
        ga[j] = c.gd[(on && f0) ? (f0 & 0x3fffu) - 1 : 0u];
        gb[j] = c.gd[(on && f1) ? (f1 & 0x3fffu) - 1 : 0u];
      }
      SPICEY_UNROLL
      for (int j = 0; j < Regs::NDD; j++) {
        uint32_t dd = rr.dd[j];
        SPICEY_OPAQUE(dd);
        if (dd >> 31) continue;
        const uint32_t f0 = dd & 0x7fffu, f1 = (dd >> 15) & 0x7fffu;
        double x = rr.sv[j][0];
        if (f0) x = (f0 & 0x4000u) ? x - ga[j] : x + ga[j];
        if (f1) x = (f1 & 0x4000u) ? x - gb[j] : x + gb[j];
        if (dd & (1u << 30)) {
          if (fabs(x) < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
          x = spicey_rcp(x);
        }
        put_entry((uint32_t)(tid + j * T), 0, x);
      }
      for (int j = Regs::NDD; j < NSV; j++) {
        const int e = tid + j * T;
        if (e >= P.nDynEnt && e < P.nRestore) put_entry((uint32_t)e, 0, rr.sv[j][0]);
      }
      stamp_rest_batched(tid);
      return;
    }
    if (OS) {  // (every field names an operand — dd_slots: all conductances first, one LDS round trip, then entry by entry)
      double ga[Regs::NDD], gb[Regs::NDD];
      SPICEY_UNROLL
      for (int j = 0; j < Regs::NDD; j++) {
        uint32_t dd = rr.dd[j];
        SPICEY_OPAQUE(dd);
        if (OA) {  // (indices from the start of W: dd_addr)
          ga[j] = Op::template ld<1>(c.W, Op::index(dd & 0x3fffu), 0);
          gb[j] = Op::template ld<1>(c.W, Op::index((dd >> 15) & 0x3fffu), 0);
          continue;
        }
        ga[j] = c.gd[(size_t)(dd & 0x3fffu)];
        gb[j] = c.gd[(size_t)((dd >> 15) & 0x3fffu)];
      }
      SPICEY_UNROLL
      for (int j = 0; j < Regs::NDD; j++) {
        uint32_t dd = rr.dd[j];
        SPICEY_OPAQUE(dd);
        double x = rr.sv[j][0] + signed_by(ga[j], dd << 17);
        x = x + signed_by(gb[j], dd << 2);
        if (dd >> 31) continue;
        if (dd & (1u << 30)) {
          if (fabs(x) < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
          x = spicey_rcp(x);
        }
        put_entry((uint32_t)(tid + j * T), 0, x);
      }
    } else
    for (int j = 0; j < Regs::NDD; j++) {
      const uint32_t e = (uint32_t)(tid + j * T);
      uint32_t dd = rr.dd[j];
      SPICEY_OPAQUE(dd);
      if (SPICEY_WAVE_ANY((dd & 0x7fffffffu) != 0u)) {  // dynamic entries are numbered first: only the first slot(s) take this path
        if (!(dd >> 31)) stamp_entry(e, dd, rr.sv[j]);
      } else if (!(dd >> 31)) {
        for (int k = 0; k < K; k++) put_entry(e, k, rr.sv[j][k]);
      }
    }
    for (int j = Regs::NDD; j < NSV; j++) {  // plain restores (a dynamic entry this far up is left to the loop below)
      const int e = tid + j * T;
      if (e >= P.nDynEnt && e < n_stamped())
        for (int k = 0; k < K; k++) put_entry((uint32_t)e, k, rr.sv[j][k]);
    }
    SPICEY_MARK(c, 8);
    if (!(brem & (16u | 1u | 2u))) return;
    SPICEY_COLD_ARGS;
    if (brem & 16u)
    SPICEY_NOUNROLL
    for (int e = tid + Regs::NDD * T; e < P.nDynEnt; e += T) {  // dynamic entries beyond the descriptor slots
      const uint32_t dd = P.ent_dd[e];
      if (dd >> 31) continue;
      double sv[K];
      for (int k = 0; k < K; k++) sv[k] = R.statv[(size_t)c.inst[k] * P.nLU + e];
      stamp_entry((uint32_t)e, dd, sv);
    }
    if (brem & 1u)
    SPICEY_NOUNROLL
    for (int e = tid + NSV * T, ne = n_stamped(); e < ne; e += T) {  // entries beyond the resident capacity
      if (e < P.nDynEnt) continue;  // done above
      const uint32_t dd = P.ent_dd[e];
      if (dd >> 31) continue;
      double sv[K];
      for (int k = 0; k < K; k++) sv[k] = R.statv[(size_t)c.inst[k] * P.nLU + e];
      stamp_entry((uint32_t)e, dd, sv);
    }
    if (brem & 2u)
    SPICEY_NOUNROLL
    for (int t = tid; t < P.nDynX; t += T) {  // entries with > 2 dynamic stamps
      const uint32_t et = P.dynx_ent[t], e = SPICEY_IDX(et);
      for (int k = 0; k < K; k++) {
        double v = R.statv[(size_t)c.inst[k] * P.nLU + e];
        for (uint32_t j = P.dynx_ptr[t]; j < P.dynx_ptr[t + 1]; j++) {
          const uint32_t ix = P.dynx_idx[j];
          const double g = c.gd[(size_t)SPICEY_IDX(ix) * K + k];
          v = (ix & SPICEY_NEG) ? v - g : v + g;
        }
        if (et & SPICEY_TGT_RECIP) {
          if (fabs(v) < SPICEY_EPS && c.valid[k]) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
          v = spicey_rcp(v);
        }
        put_entry(e, k, v);
      }
    }
  }
  SPICEY_HD void rhs_rows(int tid, Regs &rr) const {
    SPICEY_MARK(c, 9);
    if (HYB) {  // (the contributions of all resident rows in one round trip to the global element vector)
      double t[NEL][4];
      SPICEY_UNROLL
      for (int j = 0; j < NEL; j++) {
        uint32_t d0 = rr.rhs[j][0], d1 = rr.rhs[j][1];
        SPICEY_OPAQUE(d0); SPICEY_OPAQUE(d1);
        const bool on = d1 != 0xFFFFFFFFu;
        const uint32_t f[4] = {d0 & 0xffffu, d0 >> 16, d1 & 0xffffu, d1 >> 16};
        SPICEY_UNROLL
        for (int i = 0; i < 4; i++) t[j][i] = c.u[(on && f[i]) ? (f[i] & 0x7fffu) - 1 : 0u];
      }
      SPICEY_UNROLL
      for (int j = 0; j < NEL; j++) {
        uint32_t d0 = rr.rhs[j][0], d1 = rr.rhs[j][1];
        SPICEY_OPAQUE(d0); SPICEY_OPAQUE(d1);
        if (d1 == 0xFFFFFFFFu) continue;
        const uint32_t f[4] = {d0 & 0xffffu, d0 >> 16, d1 & 0xffffu, d1 >> 16};
        double acc = 0.0;
        SPICEY_UNROLL
        for (int i = 0; i < 4; i++)
          if (f[i]) acc = (f[i] & 0x8000u) ? acc - t[j][i] : acc + t[j][i];
        c.W[(size_t)(P.xoff + tid + j * T)] = acc;
      }
    } else if (OS) {  // (every field names an operand — rhs_slots: the contributions of all resident rows in one LDS round trip)
      double t[NEL][4];
      SPICEY_UNROLL
      for (int j = 0; j < NEL; j++) {
        uint32_t d0 = rr.rhs[j][0], d1 = rr.rhs[j][1];
        SPICEY_OPAQUE(d0); SPICEY_OPAQUE(d1);
        if (OA) {  // (indices from the start of W: rhs_addr)
          t[j][0] = Op::template ld<1>(c.W, Op::index(d0 & 0x3fffu), 0); t[j][1] = Op::template ld<1>(c.W, Op::index((d0 >> 16) & 0x3fffu), 0);
          t[j][2] = Op::template ld<1>(c.W, Op::index(d1 & 0x3fffu), 0); t[j][3] = Op::template ld<1>(c.W, Op::index((d1 >> 16) & 0x3fffu), 0);
          continue;
        }
        t[j][0] = c.u[(size_t)(d0 & 0x3fffu)]; t[j][1] = c.u[(size_t)((d0 >> 16) & 0x3fffu)];
        t[j][2] = c.u[(size_t)(d1 & 0x3fffu)]; t[j][3] = c.u[(size_t)((d1 >> 16) & 0x3fffu)];
      }
      SPICEY_UNROLL
      for (int j = 0; j < NEL; j++) {
        uint32_t d0 = rr.rhs[j][0], d1 = rr.rhs[j][1];
        SPICEY_OPAQUE(d0); SPICEY_OPAQUE(d1);
        if (d1 & 0x40000000u) continue;
        double acc = 0.0;
        acc = acc + signed_by(t[j][0], d0 << 16);
        acc = acc + signed_by(t[j][1], d0);
        acc = acc + signed_by(t[j][2], d1 << 16);
        acc = acc + signed_by(t[j][3], d1);
        c.W[(size_t)(P.xoff + tid + j * T)] = acc;
      }
    } else
    for (int j = 0; j < NEL; j++) {
      uint32_t d0 = rr.rhs[j][0], d1 = rr.rhs[j][1];
      SPICEY_OPAQUE(d0); SPICEY_OPAQUE(d1);
      if (d1 != 0xFFFFFFFFu) rhs_row((uint32_t)(tid + j * T), d0, d1);
    }
    SPICEY_MARK(c, 10);
    if (HYB && (brem & 4u)) rhs_rest_batched(tid);
    if (!(brem & (HYB ? 8u : 12u))) return;
    SPICEY_COLD_ARGS;
    if (!HYB && (brem & 4u))
    SPICEY_NOUNROLL
    for (int r = tid + NEL * T; r < P.n; r += T) {
      const uint32_t d0 = P.row_desc[(size_t)r * 2], d1 = P.row_desc[(size_t)r * 2 + 1];
      if (d1 != 0xFFFFFFFFu) rhs_row((uint32_t)r, d0, d1);
    }
    if (brem & 8u)
    SPICEY_NOUNROLL
    for (int t = tid; t < P.nRowX; t += T) {  // rows with > 4 contributions: +-1 gather from the CSR lists
      const uint32_t r = P.rowx[t];
      for (int k = 0; k < K; k++) {
        double acc = 0.0;
        for (uint32_t j = P.rhs_ptr[r]; j < P.rhs_ptr[r + 1]; j++) {
          const uint32_t ix = P.rhs_idx[j];
          const double t2 = c.u[(size_t)SPICEY_IDX(ix) * K + k];
          acc = (ix & SPICEY_NEG) ? acc - t2 : acc + t2;
        }
        c.W[(size_t)(P.xoff + r) * K + k] = acc;
      }
    }
  }

  SPICEY_HD void a_reiterate(int tid) const {  // iteration >= 1: diodes from x, switches from their new state
    const int oD = P.nC + P.nL + P.nV;
    for (int k = 0; k < K; k++) {
      const size_t in = (size_t)c.inst[k];
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nS; i += T)
        c.gd[(size_t)i * K + k] = spicey_switch_g(c.ison[(size_t)i * K + k], R.S_ron[in * P.nS + i], R.S_roff[in * P.nS + i]);
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nD; i += T) {
        const double *dp = R.dpar + (in * P.nD + i) * 2;
        double g2, q, irec;
        const double vd = dv16(P.D_ab[i], k);
        spicey_diode_k<FRESH>(vd, R.D_is[in * P.nD + i], dp[0], dp[1], false, g2, q, irec);
        c.gd[(size_t)(P.nS + i) * K + k] = g2;
        c.u[(size_t)(oD + i) * K + k] = q;
        if (DIAG && R.lin_vd && c.valid[k]) R.lin_vd[in * P.nD + i] = vd;
      }
    }
  }

  // ---- Z: record, update state, evaluate the next step's companions --------------------------------
  SPICEY_HD void z_cap(int i, double dv, int k, size_t in, double gc, double *oi, int cC, double &vprev, bool last) const {
    if (oi) SPICEY_STREAM_STORE(&oi[cC + i], gc * (dv - vprev));
    vprev = dv;
    c.u[(size_t)i * K + k] = gc * dv;
    if (last) (RA ? spicey_pt_ptr<double>(ptab, SPICEY_PT_C_VPREV) : R.C_vprev)[in * P.nC + i] = dv;
  }
  SPICEY_HD void z_dio(int i, double vd, int k, size_t in, double is, double dp0, double dp1, double *oi, int cD, int oD, bool last) const {
    double gg, q, irec;
    spicey_diode_k<FRESH>(vd, is, dp0, dp1, oi != nullptr, gg, q, irec);
    if (oi) SPICEY_STREAM_STORE(&oi[cD + i], irec);
    c.gd[(size_t)(P.nS + i) * K + k] = gg;
    c.u[(size_t)(oD + i) * K + k] = q;
    if (last) (RA ? spicey_pt_ptr<double>(ptab, SPICEY_PT_D_VDPREV) : R.D_vdprev)[in * P.nD + i] = vd;
  }
  // OS: slot `i` of a row section that starts at the wave-uniform `row` — a 32-bit lane BYTE offset on a base in scalars
  // (OA: the offset is made opaque — where hipcc sees that it is tid x 8 it widens it to 64 bits and adds the base in vector
  // registers, one v_lshl_add_u64 per store, instead of leaving the base to the store's scalar operand)
  static SPICEY_HD double *row_at(double *row, int i) {
    uint32_t ob = (uint32_t)i * 8u;
    if (OA) SPICEY_OPAQUE(ob);
    return (double *)((char *)row + ob);
  }
  // ... and the same two element updates storing through it (`sec`: the element class's section of the current row, null: no currents wanted)
  SPICEY_HD void z_cap_at(int i, double dv, size_t in, double gc, double *sec, double &vprev, bool last) const {
    if (sec) SPICEY_STREAM_STORE(row_at(sec, i), gc * (dv - vprev));
    vprev = dv;
    c.u[(size_t)i] = gc * dv;
    if (last) (RA ? spicey_pt_ptr<double>(ptab, SPICEY_PT_C_VPREV) : R.C_vprev)[in * P.nC + i] = dv;
  }
  SPICEY_HD void z_dio_at(int i, double vd, size_t in, double is, double dp0, double dp1, double *sec, int oD, bool last) const {
    double gg, q, irec;
    spicey_diode_k<FRESH>(vd, is, dp0, dp1, sec != nullptr, gg, q, irec);
    if (sec) SPICEY_STREAM_STORE(row_at(sec, i), irec);
    c.gd[(size_t)(P.nS + i)] = gg;
    c.u[(size_t)(oD + i)] = q;
    if (last) (RA ? spicey_pt_ptr<double>(ptab, SPICEY_PT_D_VDPREV) : R.D_vdprev)[in * P.nD + i] = vd;
  }
  // diagnostics pass of Z (SpiceyRun::lin_vd set; its own loop so that the production path carries no extra state):
  // |vd(x) - vd_lin| of this thread's diodes, and the new linearisation point
  SPICEY_HD double z_lin_err(int tid, int k, size_t in) const {
    SPICEY_COLD_ARGS;
    double lerr = 0.0;
    SPICEY_NOUNROLL
    for (int i = tid; i < P.nD; i += T) {
      const double vd = dv16(P.D_ab[i], k);
      const double e = fabs(vd - R.lin_vd[in * P.nD + i]);
      lerr = e > lerr ? e : lerr;
      R.lin_vd[in * P.nD + i] = vd;
    }
    return lerr;
  }
  SPICEY_HD void z_prefetch(int tid, int64_t step, int k, Regs &rr) const {
    const size_t in = (size_t)(K == 1 ? c.inst[0] : (k == 0 ? c.inst[0] : c.inst[K - 1]));
    const double *g = R.gstat + in * P.nGstat;
    for (int j = 0; j < NEL; j++) {
      const int i = (SPICEY_EXP & 8) ? 0x7fffffff : tid + j * T;
      rr.pf[j][0] = i < P.nR ? g[i] : 0.0;
      rr.pf[j][1] = i < P.nC ? g[P.nR + i] : 0.0;
      const bool hd = i < P.nD;
      const double *dp = R.dpar + (in * P.nD + (hd ? i : 0)) * 2;
      rr.pf[j][2] = hd ? R.D_is[in * P.nD + i] : 0.0;
      rr.pf[j][3] = hd ? dp[0] : 0.0;
      rr.pf[j][4] = hd ? dp[1] : 0.0;
    }
  }
  // ---- early-prefetch builds: the record SpiceyRun::zpar ---------------------------------------------------------------
  // Prologue, after p0_gstat's barrier: every thread copies the parameters of its own resident items — exactly the doubles
  // z_prefetch reads — into its record; it alone reads them back, so nothing but program order stands between the two.
  // Rebuilt by every launch: a second run on the handle, or new element values, see fresh parameters.
  SPICEY_HD void zpar_fill(int tid) const {
    const size_t in = (size_t)c.inst[0];
    const double *g = R.gstat + in * P.nGstat;
    for (int j = 0; j < NEL; j++) {
      const int i = tid + j * T;
      double *zp = R.zpar + ((in * NEL + (size_t)j) * (size_t)T + (size_t)tid) * 5;
      const bool hd = i < P.nD;
      const double *dp = R.dpar + (in * P.nD + (hd ? i : 0)) * 2;
      zp[0] = i < P.nR ? g[i] : 0.0;
      zp[1] = i < P.nC ? g[P.nR + i] : 0.0;
      zp[2] = hd ? R.D_is[in * P.nD + i] : 0.0;
      zp[3] = hd ? dp[0] : 0.0;
      zp[4] = hd ? dp[1] : 0.0;
    }
  }
  // one wave-uniform base per j and one 32-bit lane offset: 40 contiguous bytes per item, no bound test
  // (RA: `zrec` is this instance's record — spicey_pt_rebase_ready —, a scalar base that the loads take as such; item j
  // starts j x T x 40 bytes behind it)
  static SPICEY_HD uint32_t rec_offset(int tid) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24((unsigned)tid, 40u);  // (tid < 2^24: a full-rate multiply, where the 32-bit one runs at a quarter)
#else
    return (uint32_t)tid * 40u;
#endif
  }
  SPICEY_HD void z_prefetch_rec(int tid, Regs &rr, const double *zrec = nullptr) const {
    if (RA) {
      const uint32_t ob = rec_offset(tid);
      for (int j = 0; j < NEL; j++) {
        // (item j's base is formed in scalars and stays there: base + lane offset + constant is then one addressing mode)
        uint64_t bj = (uint64_t)(uintptr_t)zrec + (uint64_t)j * (uint64_t)(uint32_t)T * 40u;
        SPICEY_OPAQUE_S(bj);
        const double *zp = (const double *)(spicey_global_ptr<const char>(bj) + ob);
        for (int q = 0; q < 5; q++) rr.pf[j][q] = (SPICEY_EXP & 8) ? 0.0 : zp[q];
      }
      return;
    }
    const uint32_t ob = (uint32_t)tid * 40u;  // (a BYTE offset of 32 bits: base in scalars + this + a constant is one addressing mode)
    for (int j = 0; j < NEL; j++) {
      const char *base = (const char *)(R.zpar + ((size_t)c.inst[0] * NEL + (size_t)j) * (size_t)T * 5);
      const double *zp = (const double *)(base + ob);
      for (int q = 0; q < 5; q++) rr.pf[j][q] = (SPICEY_EXP & 8) ? 0.0 : zp[q];
    }
  }
  // the early fetch: Z's parameters and the next step's source value, with the backward phases to arrive in
  SPICEY_HD void z_early(int tid, int64_t step, Regs &rr) const {
    if (RA) {  // (R.zpar, R.src: this instance's — spicey_pt_args_early)
      z_prefetch_rec(tid, rr, R.zpar);
      rr.srcn = z_src_fetch_at(tid, step, R.src);
      return;
    }
    z_prefetch_rec(tid, rr);
    rr.srcn = z_src_fetch(tid, step, (size_t)c.inst[0]);
  }
  // the same registers left UNDEFINED where nothing will read them before they are written again (Z then fetches for itself): a definition on this path for the compiler — so that the values are not
  // live around the time loop — that costs no instruction.  The host's executors get NaN.
  SPICEY_HD void z_early_none(Regs &rr) const {
    for (int j = 0; j < NEL; j++)
      for (int q = 0; q < 5; q++) spicey_undef(rr.pf[j][q]);
    spicey_undef(rr.srcn);
  }
  static SPICEY_HD void spicey_undef(double &x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "=v"(x));
#else
    x = NAN;
#endif
  }
  // next step's source values: issued before the tasks of the last backward phase, parked in LDS after them
  SPICEY_HD double z_src_fetch(int tid, int64_t step, size_t in) const {
    return (tid < P.nV && step != R.steps) ? R.src[in * R.src_stride + (size_t)(step + 1) * P.nV + tid] : 0.0;
  }
  // RA: from the instance's own table `srcb`; (step + 1) x nV as one 32 x 32 -> 64-bit product (spicey_ready_steps_ok)
  static SPICEY_HD uint64_t mul32(uint32_t a, uint32_t b) { return (uint64_t)a * (uint64_t)b; }
  SPICEY_HD double z_src_fetch_at(int tid, int64_t step, const double *srcb) const {
    const uint32_t nxt = (uint32_t)SPICEY_UNIFORM((int)((uint32_t)step + 1u));
    return (tid < P.nV && step != R.steps) ? *row_at(const_cast<double *>(srcb) + mul32(nxt, (uint32_t)P.nV), tid) : 0.0;
  }
  SPICEY_HD void z_src_park(int tid, double v) const {
    if (tid < P.nV) c.u[(size_t)(P.nC + P.nL + P.nV + P.nD + tid) * K] = v;
  }
  SPICEY_HD void z_prefetch_none(Regs &rr) const {
    for (int j = 0; j < NEL; j++)
      for (int q = 0; q < 5; q++) rr.pf[j][q] = 0.0;
  }
  SPICEY_HD void z_record(int tid, int64_t step, Regs &rr, bool prefetched) const {
    const bool last = step == R.steps;
    const uint32_t st32 = (uint32_t)SPICEY_UNIFORM((int)(uint32_t)step);  // (RA: the low word of the step, for the 32 x 32 -> 64-bit row offsets)
    (void)st32;
    const int oL = P.nC, oV = P.nC + P.nL, oD = P.nC + P.nL + P.nV;
    const int cR = 0, cC = P.nR, cL = P.nR + P.nC, cV = cL + P.nL, cS = cV + P.nV, cD = cS + P.nS;
    if constexpr (SF) {
      // The early fetch is waited for HERE, on every path through this phase and in front of its first result store.  The wait
      // below stands behind the test of `valid`; the path around it would leave the loads in flight for the compiler, and the
      // second phase, which reads the same registers, would wait for vmcnt behind this phase's stores in every step.
      for (int j = 0; j < NEL; j++)
        for (int q = 0; q < 5; q++) SPICEY_OPAQUE(rr.pf[j][q]);
      SPICEY_OPAQUE(rr.srcn);  // (fetched with them; this phase overwrites it with the row of the thread's source)
    }
    // The instance loop is kept ROLLED here (one copy of the exp / store code, one instance's working set):
    // unrolled and interleaved it needs ~2x the VGPRs and the register-resident program spills.
    SPICEY_NOUNROLL
    for (int k = 0; k < K; k++) {
      const int vk = K == 1 ? c.valid[0] : (k == 0 ? c.valid[0] : c.valid[K - 1]);
      if (!vk) continue;
      const size_t in = (size_t)(K == 1 ? c.inst[0] : (k == 0 ? c.inst[0] : c.inst[K - 1]));
      // (OS: the table's two result pointers are this instance's row 0 already — spicey_pt_rebase_rows)
      double *ov = RA ? R.out_v + mul32(st32, (uint32_t)P.nOut) : R.out_v + ((OS ? 0 : in * (size_t)(R.steps + 1)) + (size_t)step) * P.nOut;
      double *oi = R.out_i ? (RA ? R.out_i + mul32(st32, (uint32_t)P.nCur) : R.out_i + ((OS ? 0 : in * (size_t)(R.steps + 1)) + (size_t)step) * P.nCur) : nullptr;
      const double *gh = RA ? nullptr : R.gstat + in * P.nGstat;  // (only the beyond-capacity loops read it: RA forms it there)
      if (DIAG && R.lin_vd) {  // diagnostics (wave-uniform): the step's one-shot linearisation error
        const double lerr = z_lin_err(tid, k, in);
        if (R.lin_err) spicey_lin_err_report(R, in, step, tid, lerr);
      }
      SPICEY_MARK(c, 15);
      // Element parameters of the resident items come from L2: all their loads are issued together (one round
      // trip per step instead of one per element section), normally already during the last backward phase.
      if (!(K == 1 && prefetched)) {
        if (RA) z_prefetch_rec(tid, rr, spicey_pt_ptr<const double>(ptab, SPICEY_PT_ZPAR));
        else if (EP) z_prefetch_rec(tid, rr);
        else z_prefetch(tid, step, k, rr);
      }
      double pR[NEL], pC[NEL], pIs[NEL], pD0[NEL], pD1[NEL];
      for (int j = 0; j < NEL; j++) { pR[j] = rr.pf[j][0]; pC[j] = rr.pf[j][1]; pIs[j] = rr.pf[j][2]; pD0[j] = rr.pf[j][3]; pD1[j] = rr.pf[j][4]; }
      double srcn = (K == 1 && prefetched) ? 0.0 : RA ? z_src_fetch_at(tid, step, spicey_pt_ptr<const double>(ptab, SPICEY_PT_SRC)) : z_src_fetch(tid, step, in);
      // ... and all of them are WAITED for here, before the first result store is issued: gfx9 has one counter
      // (vmcnt) for loads and stores, which may complete out of order, so once a store is in flight a wait for any
      // load becomes vmcnt(0) = "until every result store has been acknowledged" (~1 us each time).
      for (int j = 0; j < NEL; j++) { SPICEY_OPAQUE(pR[j]); SPICEY_OPAQUE(pC[j]); SPICEY_OPAQUE(pIs[j]); SPICEY_OPAQUE(pD0[j]); SPICEY_OPAQUE(pD1[j]); }
      SPICEY_OPAQUE(srcn);
      SPICEY_MARK(c, 0);
      if (tid < P.nV) {  // source tid: branch current out, next step's value in (read by the next B only)
        uint32_t vx = rr.ox[0];
        SPICEY_OPAQUE(vx);
        if (oi) oi[cV + tid] = OA ? volt_res<1>(vx) : c.W[(size_t)(vx >> 16) * K + k];
        if constexpr (SF) {  // (the source's row, 0.0 + its next value as rhs_rows forms it, waits in the source register for the second phase)
          if (!last) srcn = 0.0 + ((K == 1 && prefetched) ? c.u[(size_t)(oD + P.nD + tid) * K + k] : srcn);
        } else
        if (!last) c.u[(size_t)(oV + tid) * K + k] = (K == 1 && prefetched) ? c.u[(size_t)(oD + P.nD + tid) * K + k] : srcn;
      }
      if constexpr (SF) rr.srcn = srcn;  // (defined on every path; read by the second phase only where the thread has a source's row and a step follows)
      SPICEY_SCHED_FENCE;
      // resident items (element / row / output tid + j T).  All their terminal voltages are read first, back to
      // back (one LDS round trip), then class by class so that the parameter registers die early.
      {
        double vo[NEL], dR[NEL];
        for (int j = 0; j < NEL; j++) {
          uint32_t ox = rr.ox[j], eR = rr.eR[j];
          SPICEY_OPAQUE(ox); SPICEY_OPAQUE(eR);
          vo[j] = OS ? volt_res<0>(ox) : volt16(ox & 0xFFFFu, k);
          dR[j] = OS ? dv_res(eR) : dv16(eR, k);
        }
        SPICEY_SCHED_FENCE;
        for (int j = 0; j < NEL; j++) {
          const int i = tid + j * T;
          if (OS) {
            if (i < P.nOut && !(SPICEY_EXP & 16)) SPICEY_STREAM_STORE(row_at(ov, i), vo[j]);
            if (oi && i < P.nR && !(SPICEY_EXP & 16)) SPICEY_STREAM_STORE(row_at(oi + cR, i), dR[j] * pR[j]);
            continue;
          }
          if (i < P.nOut && !(SPICEY_EXP & 16)) SPICEY_STREAM_STORE(&ov[i], vo[j]);
          if (oi && i < P.nR && !(SPICEY_EXP & 16)) SPICEY_STREAM_STORE(&oi[cR + i], dR[j] * pR[j]);
        }
        SPICEY_SCHED_FENCE;
      }
      double dC[NEL], dD[NEL];
      for (int j = 0; j < NEL; j++) {
        uint32_t eC = rr.eC[j], eD = rr.eD[j];
        SPICEY_OPAQUE(eC); SPICEY_OPAQUE(eD);
        dC[j] = OS ? dv_res(eC) : dv16(eC, k);
        dD[j] = OS ? dv_res(eD) : dv16(eD, k);
      }
      SPICEY_SCHED_FENCE;
      SPICEY_MARK(c, 1);
      if constexpr (SF) {
        // every LDS read of the solution is done.  The capacitors and the diodes — z_cap_at and z_dio_at without their LDS
        // writes (-0.0, the neutral operand, where there is no such element) —, and from their values, in registers, the
        // next step's stamps: stamp_matrix's and rhs_rows' sums, operation for operation.  The entries go straight into W:
        // nothing reads a matrix entry between K_0's barrier and U_0.  The rows wait in pf[j][0] for the second phase.  Nothing
        // is stamped behind the last step: no flag is raised for a matrix that no step solves.
        double gcv[NEL];
        for (int j = 0; j < NEL; j++) {
          const int i = tid + j * T;
          gcv[j] = -0.0;
          if (i < P.nC) {
            if (oi) SPICEY_STREAM_STORE(row_at(oi + cC, i), pC[j] * (dC[j] - rr.vprev[j][0]));
            rr.vprev[j][0] = dC[j];
            gcv[j] = pC[j] * dC[j];
            if (last) (RA ? spicey_pt_ptr<double>(ptab, SPICEY_PT_C_VPREV) : R.C_vprev)[in * P.nC + i] = dC[j];
          }
        }
        SPICEY_SCHED_FENCE;
        SPICEY_MARK(c, 2);
        for (int j = 0; j < NEL; j++) {
          const int i = tid + j * T;
          double gg = -0.0, q = -0.0;
          if (i < P.nD) {
            double irec;
            spicey_diode_k<FRESH>(dD[j], pIs[j], pD0[j], pD1[j], oi != nullptr, gg, q, irec);
            if (oi) SPICEY_STREAM_STORE(row_at(oi + cD, i), irec);
            if (last) (RA ? spicey_pt_ptr<double>(ptab, SPICEY_PT_D_VDPREV) : R.D_vdprev)[in * P.nD + i] = dD[j];
          }
          double acc = 0.0;
          if (!last) {
            uint32_t e = rr.dd[j], r = rr.rhs[j][0];
            SPICEY_OPAQUE(e); SPICEY_OPAQUE(r);
            double x = rr.sv[j][0] + sf_operand(gg, e, SPICEY_SF_F0);
            x = x + sf_operand(gg, e, SPICEY_SF_F1);
            if (!(e & SPICEY_SF_NONE)) {
              if (e & SPICEY_SF_RECIP) {
                if (fabs(x) < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
                x = spicey_rcp(x);
              }
              Op::template st<1>(c.W, Op::template half<0>(e), 0, x);
            }
            const double a = sf_operand(gcv[j], r, SPICEY_SF_F0), b = sf_operand(q, r, SPICEY_SF_F1);
            const bool swap = (r & SPICEY_SF_SWAP) != 0u;
            acc = acc + (swap ? b : a);
            acc = acc + (swap ? a : b);
          }
          rr.pf[j][0] = acc;
          SPICEY_SCHED_FENCE;
        }
        SPICEY_MARK(c, 3);
        continue;
      }
      for (int j = 0; j < NEL; j++) {
        const int i = tid + j * T;
        if (i < P.nC && !(SPICEY_EXP & 4)) {
          double vp = K == 1 ? rr.vprev[j][0] : (k == 0 ? rr.vprev[j][0] : rr.vprev[j][K - 1]);
          if (OS) z_cap_at(i, dC[j], in, pC[j], oi ? oi + cC : nullptr, vp, last);
          else z_cap(i, dC[j], k, in, pC[j], oi, cC, vp, last);
          if (K == 1 || k == 0) rr.vprev[j][0] = vp;
          else rr.vprev[j][K - 1] = vp;
        }
      }
      SPICEY_SCHED_FENCE;
      SPICEY_MARK(c, 2);
      for (int j = 0; j < NEL; j++) {
        const int i = tid + j * T;
        if (i < P.nD && !(SPICEY_EXP & 2)) {
          if (OS) z_dio_at(i, dD[j], in, pIs[j], pD0[j], pD1[j], oi ? oi + cD : nullptr, oD, last);
          else z_dio(i, dD[j], k, in, pIs[j], pD0[j], pD1[j], oi, cD, oD, last);
        }
        SPICEY_SCHED_FENCE;
      }
      SPICEY_MARK(c, 3);
      if ((SPICEY_EXP & 32) || !zrem) continue;
      SPICEY_COLD_ARGS;
      const double *g = RA ? R.gstat + in * P.nGstat : gh;
      if (HYB) {
        // (hybrid workspace: four items of every kind at a time — indices and parameters of all four in flight before the
        // first terminal voltage is read; the same arithmetic per item as the loops below)
        if (zrem & 1u)
        SPICEY_NOUNROLL
        for (int i0 = tid + NEL * T; i0 < P.nOut; i0 += BW * T) {
          int32_t xi[BW];
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) xi[b] = P.out_x[i0 + b * T < P.nOut ? i0 + b * T : i0];
          double v[BW];
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) v[b] = xi[b] < 0 ? 0.0 : c.W[(size_t)xi[b]];
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++)
            if (i0 + b * T < P.nOut) SPICEY_STREAM_STORE(&ov[i0 + b * T], v[b]);
        }
        if (oi && (zrem & 2u))
        SPICEY_NOUNROLL
        for (int i0 = tid + NEL * T; i0 < P.nR; i0 += BW * T) {
          uint32_t ab[BW];
          double gg[BW], dv[BW];
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) { const int i = i0 + b * T < P.nR ? i0 + b * T : i0; ab[b] = P.R_ab[i]; gg[b] = g[i]; }
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) dv[b] = dv16(ab[b], k);
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++)
            if (i0 + b * T < P.nR) SPICEY_STREAM_STORE(&oi[cR + i0 + b * T], dv[b] * gg[b]);
        }
        if (zrem & 4u)
        SPICEY_NOUNROLL
        for (int i0 = tid + NEL * T; i0 < P.nC; i0 += BW * T) {  // beyond the resident capacity: vPrev lives in the state array
          uint32_t ab[BW];
          double gc[BW], vp[BW], dv[BW];
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) {
            const int i = i0 + b * T < P.nC ? i0 + b * T : i0;
            ab[b] = P.C_ab[i]; gc[b] = g[P.nR + i]; vp[b] = R.C_vprev[in * P.nC + i];
          }
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) dv[b] = dv16(ab[b], k);
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) {
            const int i = i0 + b * T;
            if (i >= P.nC) continue;
            z_cap(i, dv[b], k, in, gc[b], oi, cC, vp[b], false);
            R.C_vprev[in * P.nC + i] = vp[b];
          }
        }
        if (zrem & 64u)
        SPICEY_NOUNROLL
        for (int i0 = tid + NEL * T; i0 < P.nD; i0 += BW * T) {
          uint32_t ab[BW];
          double is4[BW], d0[BW], d1[BW], vd[BW];
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) {
            const int i = i0 + b * T < P.nD ? i0 + b * T : i0;
            const double *dp = R.dpar + (in * P.nD + i) * 2;
            ab[b] = P.D_ab[i]; is4[b] = R.D_is[in * P.nD + i]; d0[b] = dp[0]; d1[b] = dp[1];
          }
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++) vd[b] = dv16(ab[b], k);
          SPICEY_UNROLL
          for (int b = 0; b < BW; b++)
            if (i0 + b * T < P.nD) z_dio(i0 + b * T, vd[b], k, in, is4[b], d0[b], d1[b], oi, cD, oD, last);
        }
      }
      if (!HYB && (zrem & 1u))
      SPICEY_NOUNROLL
      for (int i = tid + NEL * T; i < P.nOut; i += T) ov[i] = P.out_x[i] < 0 ? 0.0 : c.W[(size_t)P.out_x[i] * K + k];
      if (!HYB && oi && (zrem & 2u)) {
        SPICEY_NOUNROLL
        for (int i = tid + NEL * T; i < P.nR; i += T) oi[cR + i] = dv16(P.R_ab[i], k) * g[i];
      }
      if (!HYB && (zrem & 4u))
      SPICEY_NOUNROLL
      for (int i = tid + NEL * T; i < P.nC; i += T) {  // beyond the resident capacity: vPrev lives in the state array
        double vp = R.C_vprev[in * P.nC + i];
        z_cap(i, dv16(P.C_ab[i], k), k, in, g[P.nR + i], oi, cC, vp, false);
        R.C_vprev[in * P.nC + i] = vp;
      }
      if (zrem & 8u)
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nL; i += T) {
        const double dv = dv16(P.L_ab[i], k);
        const double il = g[P.nR + P.nC + i] * dv + c.u[(size_t)(oL + i) * K + k];
        if (oi) oi[cL + i] = il;
        c.u[(size_t)(oL + i) * K + k] = il;
        if (last) R.L_iprev[in * P.nL + i] = il;
      }
      if (zrem & 16u)
      SPICEY_NOUNROLL
      for (int i = tid + T; i < P.nV; i += T) {
        if (oi) oi[cV + i] = c.W[(size_t)P.V_x[i] * K + k];
        if (!last) c.u[(size_t)(oV + i) * K + k] = R.src[in * R.src_stride + (size_t)(step + 1) * P.nV + i];
      }
      if (zrem & 32u)
      SPICEY_NOUNROLL
      for (int i = tid; i < P.nS; i += T) {
        const int on = c.ison[(size_t)i * K + k];
        const double gs = spicey_switch_g(on, R.S_ron[in * P.nS + i], R.S_roff[in * P.nS + i]);
        const double va = P.S_a[i] < 0 ? 0.0 : c.W[(size_t)P.S_a[i] * K + k], vb = P.S_b[i] < 0 ? 0.0 : c.W[(size_t)P.S_b[i] * K + k];
        if (oi) oi[cS + i] = (va - vb) * gs;
        c.gd[(size_t)i * K + k] = gs;
        if (last) R.S_ison[in * P.nS + i] = on;
      }
      if (!HYB && (zrem & 64u))
      SPICEY_NOUNROLL
      for (int i = tid + NEL * T; i < P.nD; i += T) {
        const double *dp = R.dpar + (in * P.nD + i) * 2;
        z_dio(i, dv16(P.D_ab[i], k), k, in, R.D_is[in * P.nD + i], dp[0], dp[1], oi, cD, oD, last);
      }
      SPICEY_SCHED_FENCE;
    }
  }

  // ---- SF: the stamp fuse ------------------------------------------------------------------------------------------------
  // Prologue, behind the phase that stamped step 0 with today's B: the descriptor registers take the thread's four slot
  // words of the host's table, the static values those of the entries the slots name (per instance, as ever: statv by
  // entry id).  Nothing of the old dealing stays: the same registers, other contents.
  SPICEY_HD void sf_load(int tid, Regs &rr, const uint32_t *table) const {
    const uint32_t *w = table + (size_t)tid * SPICEY_STAMP_FUSE_THREAD_WORDS;
    for (int j = 0; j < 2; j++) {
      const uint32_t e = w[j], r = w[2 + j];
      rr.dd[j] = e;
      rr.rhs[j][0] = r;
      rr.rhs[j][1] = j == 0 ? w[4] : 0u;  // ([0][1]: the row of source tid)
      rr.sv[j][0] = (e & SPICEY_SF_NONE) ? 0.0 : R.statv[(size_t)c.inst[0] * P.nLU + (e & 0xffffu)];
    }
    // ... and all of them are WAITED for here, once per run.  Their first use is in the second phase of Z; a load that the
    // compiler still counts as in flight there costs every step a wait for vmcnt, which by then holds the first phase's
    // result stores (z_record has the story: ~1 us each time).
    for (int j = 0; j < 2; j++) { SPICEY_OPAQUE(rr.dd[j]); SPICEY_OPAQUE(rr.rhs[j][0]); SPICEY_OPAQUE(rr.rhs[j][1]); SPICEY_OPAQUE(rr.sv[j][0]); }
  }
  // operand `g` as a slot word's two flag bits at `has` say: absent reads -0.0, the neutral element, as an empty field did
  static SPICEY_HD double sf_operand(double g, uint32_t w, uint32_t has) {
    const double s = signed_by(g, (w & (has << 1)) ? 0x80000000u : 0u);
    return (w & has) ? s : -0.0;
  }
  // The second phase of Z, behind the barrier that follows the first: every reader of the solution has read, and the rows of
  // the next right-hand side — formed by the first phase, waiting in registers — go over it.  No argument of the run is
  // read here: the slot words say what the thread has to write.
  SPICEY_HD void z_fuse(int tid, bool last, Regs &rr) const {
    if (tid == 0) c.flags[0] = 0;
    rr.cursor = 0;  // a new solve walks the resident slots from the start
    if (last || !c.valid[0]) return;
    for (int j = 0; j < 2; j++) {
      uint32_t r = rr.rhs[j][0];
      SPICEY_OPAQUE(r);
      if (!(r & SPICEY_SF_NONE)) Op::template st<1>(c.W, Op::template half<0>(r), 0, rr.pf[j][0]);
    }
    uint32_t sr = rr.rhs[0][1];
    SPICEY_OPAQUE(sr);
    if (!(sr & SPICEY_SF_NONE)) Op::template st<1>(c.W, Op::template half<0>(sr), 0, rr.srcn);  // (source tid's row)
  }
};
