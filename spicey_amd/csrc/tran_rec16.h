// tran_rec16.h — the 16-bit record interpreter of the v2 factor / backward phases (tran_exec.h is the map).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "program.h"
#include "tran_common.h"
#include "tran_pt.h"

// ---------------------------------------------------------------------------------------------
// v2: register-resident program.  The factor / backward task lists are step-invariant, so every
// thread keeps its share as RMAX 16-byte records in VGPRs for the whole transient (the register file,
// 512 KB per CU, is the largest low-latency store of the chip); only phases that do not fit are
// streamed from L2.  Each (wave, slot) chunk belongs to one phase, so dispatch is wave-uniform.
// Register arrays that are indexed with a wave-uniform RUNTIME index (the slot cursor): as native vector
// types hipcc addresses them through the VGPR index register (s_set_gpr_idx), O(1), instead of a compare
// chain over all slots or a scratch round trip.
#if defined(__clang__)
template <int N> struct U32Vec { typedef uint32_t type __attribute__((ext_vector_type(N))); };
#else
template <int N> struct U32Arr { uint32_t v[N]; uint32_t &operator[](int i) { return v[i]; } const uint32_t &operator[](int i) const { return v[i]; } };
template <int N> struct U32Vec { typedef U32Arr<N> type; };  // (host build: a plain array; gcc's vector types want a power of two)
#endif

// What a (RMAX, NSV, NEL) build is, for the few places where the shapes differ in kind (launch_plan.h: SPICEY_V2_SHAPES):
//   packed  the two-workgroups-per-CU builds — four slots, two elements per thread: 128 VGPRs and nothing to spare
//   fresh   the packed build that runs FRESH-FILL programs (program.h: nKeep) — two re-stamped entries per thread, both with
//           a dynamic-stamp descriptor.  Only this build decodes the fresh flags of the records and restores [0, nKeep) in
//           B: every other build is compiled exactly as without the option and never sees such a program.
template <int RMAX, int NSV, int NEL>
struct SpiceyShapeKind {
  static constexpr bool packed = RMAX == 4 && NEL == 2;
  static constexpr bool fresh = packed && NSV == 2;
};

template <int K, int RMAX, int NSV, int NEL>
struct ResRegs {
  // factor / backward task records, one 16-byte record per slot, word-major; the slots of a wave are sorted
  // by phase, `phv` holds the phase id of every slot (one byte each, 0xFF = unused), `cursor` the next slot
  typename U32Vec<RMAX>::type w0, w1, w2, w3;
  typename U32Vec<(RMAX + 3) / 4>::type phv;
  int32_t cursor;
  // entries with dynamic stamps are numbered first: only the first NDD slots can hold one and need a descriptor
  static constexpr int NDD = SpiceyShapeKind<RMAX, NSV, NEL>::packed ? 2 : NSV / 2;
  double sv[NSV][K];    // static part of the entries this thread re-stamps (e = tid + j T)
  uint32_t dd[NDD];     // dynamic-stamp descriptors of the first NDD of them
  uint32_t rhs[NEL][2]; // right-hand-side descriptors of rows tid + j T
  uint32_t eR[NEL], eC[NEL], eD[NEL], ox[NEL];  // packed terminals of elements tid + j T; W index of output tid + j T (ox[0] >> 16: source tid's branch current)
  double vprev[NEL][K]; // vPrev of capacitors tid + j T (simulateTRAN.ts:221-225), exact
  // Z's element parameters {1/R, C/dt, Is, 1/(N VT), Is/(N VT)} of items tid + j T and the next source value:
  // fetched at the end of the last backward phase so that the L2 round trip (~1900 cycles measured) overlaps that
  // phase's barrier; live only from there to Z (K == 1 geometries)
  double pf[NEL][5];
  // early-prefetch builds: the next step's value of source tid, fetched with pf between the factor and the backward phases and
  // parked in LDS at the tail of the last backward phase (TranPhases2::z_early / z_src_park); live only between the two
  double srcn;
  // fresh build: this thread's first streamed record of factor phase 0 (a 32-byte row record), fetched under phase B —
  // TranPhases2::u0_fetch writes all eight words on every path of B, spicey_uk_phase consumes them in phase 0 and clears
  // them at the end of every factor phase, so they are live from B to U_0 only.  Untouched in every other build.
  // Resident-record form of that build (tran_v2_run.h: UR): TranPhases2::load_resident fills the eight words ONCE — the
  // record is the same 32 bytes in every step of a run — a thread at or beyond the record count holds zeros (no VALID flag:
  // nothing runs), spicey_u0_resident_phase executes them in phase 0 and nothing fetches or clears them: live for the run.
  uint32_t u0[SpiceyShapeKind<RMAX, NSV, NEL>::fresh ? 8 : 1];
};

// One task.  For the common inline case (<= 2 products) ALL operands are fetched up front — unused index fields
// are 0, a valid address — and the unused products are masked by selects: one LDS round trip per task instead of
// one per product (the dependent ds_read -> wait -> fma chains dominated the small phases).
// OPG (hybrid workspace, SpiceyProg::hybrid): the phase eliminates / back-substitutes the LEAVES of the elimination tree —
// the pivot's own entries (L, reciprocal diagonal, U) are read from the global array c.G by entry id, every target and
// every right-hand-side / solution operand from LDS as always (`xoff` = first LDS index of the right-hand side: the third
// operand of a right-hand-side task is y_k, not an entry).
// `ovf()` yields the overflow list (SpiceyProg::ovf16): asked for only by a task of more than two products, so that a phase
// without one fetches nothing for it.
// FRESH (fresh-fill builds): a factor task flagged SPICEY_R16_FRESH creates its target — it starts from 0.0 and does not
// read it (the entry's static value IS 0.0, so the fma chain and its bits are those of the unflagged task).
// OA (operand-address builds, tran_common.h: SpiceyOperand): the operands of the inline case and the target are named by
// handles — one instruction from the record word to the LDS address, the target's shared by its read and its write.
// INL (the fixed-schedule build, tran_v2_run.h: FS): the host has made sure that no record this call can see has more than two
// products (launch_plan.h: spicey_fixed_schedule_fits) — the overflow path is not compiled and `ovf` never asked.
template <int K, bool KTASK, bool OPG = false, bool FRESH = false, bool OA = false, bool INL = false, class OV>
SPICEY_HD void spicey_exec_rec16(const WgCtx<K> &c, OV ovf, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3,
                                 uint32_t keep_from = 0u, uint32_t xoff = 0u) {
  static_assert(!OA || !OPG, "operand addresses: everything lives in the LDS workspace");
  typedef SpiceyOperand<OA> Op;
  const uint32_t meta = w0 >> 16;
  if (!(meta & (SPICEY_R16_VALID << 8))) return;
  const uint32_t tgt = w0 & 0xffffu, cnt = meta & 0xffu;
  const uint32_t tgt_a = OA ? Op::template half<0>(w0) : tgt;  // (the target's handle: one for its read and its write)
  // a reused factorisation (linear circuit, step > 0) runs only the right-hand-side column of the factor tasks:
  // keep_from = first right-hand-side index then, 0 otherwise
  if (!KTASK && tgt < keep_from) return;
  const double *E = OPG ? c.G : c.W;  // where the pivot's own entries are
  double acc[K];
  if (KTASK) {
    const uint32_t d = w1 & 0xffffu;
    if (INL || cnt <= 2) {
      const uint32_t u0 = Op::template half<1>(w1), x0 = Op::template half<0>(w2), u1 = Op::template half<1>(w2), x1 = Op::template half<0>(w3);
      const uint32_t d_a = OA ? Op::template half<0>(w1) : d;
      const bool two = SPICEY_WAVE_ANY(cnt == 2);  // tasks are sorted by count: most waves are uniform
      double a0[K], b0[K], a1[K], b1[K], dv[K];
      for (int k = 0; k < K; k++) {
        acc[k] = Op::template ld<K>(c.W, tgt_a, k);
        a0[k] = Op::template ld<K>(E, u0, k); b0[k] = Op::template ld<K>(c.W, x0, k);
        dv[k] = Op::template ld<K>(E, d_a, k);
      }
      if (two)
        for (int k = 0; k < K; k++) { a1[k] = Op::template ld<K>(E, u1, k); b1[k] = Op::template ld<K>(c.W, x1, k); }
      for (int k = 0; k < K; k++) {  // explicit fma: the same rounding in every interpreter and geometry
        const double s0 = fma(-a0[k], b0[k], acc[k]);
        acc[k] = cnt >= 1 ? s0 : acc[k];
        if (two) {
          const double s1 = fma(-a1[k], b1[k], acc[k]);
          acc[k] = cnt == 2 ? s1 : acc[k];
        }
        acc[k] *= dv[k];
      }
    } else {
      for (int k = 0; k < K; k++) acc[k] = Op::template ld<K>(c.W, tgt_a, k);
      const uint16_t *o = ovf() + w3;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t u = o[2 * j], x = o[2 * j + 1];
        for (int k = 0; k < K; k++) acc[k] = fma(-E[(size_t)u * K + k], c.W[(size_t)x * K + k], acc[k]);
      }
      for (int k = 0; k < K; k++) acc[k] *= E[(size_t)d * K + k];
    }
    for (int k = 0; k < K; k++) Op::template st<K>(c.W, tgt_a, k, acc[k]);
  } else {
    // (hybrid: the third operand is an entry of the pivot's U row — global — for a matrix target, y_k — LDS — for a
    // right-hand-side target)
    const bool third_lds = !OPG || tgt >= xoff;
    const bool keep_old = !FRESH || !(meta & (SPICEY_R16_FRESH << 8));
    if (INL || cnt <= 2) {
      const uint32_t l0 = Op::template half<0>(w1), d0 = Op::template half<1>(w1), u0 = Op::template half<0>(w2);
      const uint32_t l1 = Op::template half<1>(w2), d1 = Op::template half<0>(w3), u1 = Op::template half<1>(w3);
      const bool two = SPICEY_WAVE_ANY(cnt == 2);
      double p0[K], q0[K], r0[K], p1[K], q1[K], r1[K];
      for (int k = 0; k < K; k++) {
        acc[k] = 0.0;
        if (keep_old) acc[k] = Op::template ld<K>(c.W, tgt_a, k);
        p0[k] = Op::template ld<K>(E, l0, k); q0[k] = Op::template ld<K>(E, d0, k);
        r0[k] = (!OPG || third_lds) ? Op::template ld<K>(c.W, u0, k) : c.G[(size_t)u0 * K + k];
      }
      if (two)
        for (int k = 0; k < K; k++) {
          p1[k] = Op::template ld<K>(E, l1, k); q1[k] = Op::template ld<K>(E, d1, k);
          r1[k] = (!OPG || third_lds) ? Op::template ld<K>(c.W, u1, k) : c.G[(size_t)u1 * K + k];
        }
      for (int k = 0; k < K; k++) {
        const double s0 = fma(-(p0[k] * q0[k]), r0[k], acc[k]);
        acc[k] = cnt >= 1 ? s0 : acc[k];
        if (two) {
          const double s1 = fma(-(p1[k] * q1[k]), r1[k], acc[k]);
          acc[k] = cnt == 2 ? s1 : acc[k];
        }
      }
    } else {
      for (int k = 0; k < K; k++) {
        acc[k] = 0.0;
        if (keep_old) acc[k] = Op::template ld<K>(c.W, tgt_a, k);
      }
      const uint16_t *o = ovf() + w3;
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t l = o[3 * j], d = o[3 * j + 1], u = o[3 * j + 2];
        for (int k = 0; k < K; k++) {
          const double uv = (!OPG || third_lds) ? c.W[(size_t)u * K + k] : c.G[(size_t)u * K + k];
          acc[k] = fma(-(E[(size_t)l * K + k] * E[(size_t)d * K + k]), uv, acc[k]);
        }
      }
    }
    if (meta & (SPICEY_R16_RECIP << 8)) {
      for (int k = 0; k < K; k++) {
        if (fabs(acc[k]) < SPICEY_EPS && c.valid[k]) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
        acc[k] = spicey_rcp(acc[k]);
      }
    }
    for (int k = 0; k < K; k++) Op::template st<K>(c.W, tgt_a, k, acc[k]);
  }
}

// One ROW record of a factor phase (program.h: fus16): the targets a_ii, y_i and the (at most two) fills of row i from its
// (at most two) pivots of this level, sharing the multipliers -(L_ik d_k).  The products and their order are those of the
// generic tasks it stands for.  rhs_only: a reused factorisation updates y_i alone.
// FRESH: a fill target flagged SPICEY_ROW_FRESH_* is created here — started from 0.0, not read.
// OA: every operand by its handle (tran_common.h: SpiceyOperand) — 14 addresses, one instruction each; the four targets'
// are shared by their reads and writes.
template <int K, bool OPG = false, bool FRESH = false, bool OA = false>
SPICEY_HD void spicey_exec_row16(const WgCtx<K> &c, const uint32_t *w, bool rhs_only) {
  static_assert(!OA || !OPG, "operand addresses: everything lives in the LDS workspace");
  typedef SpiceyOperand<OA> Op;
  const double *E = OPG ? c.G : c.W;  // (hybrid workspace: the pivots' own entries L_ik, d_k, U_ki, U_k,o come from the global array)
  const uint32_t meta = w[0] >> 16;
  if (!(meta & (SPICEY_R16_VALID << 8))) return;
  const uint32_t iaa = Op::template half<0>(w[0]), iy = Op::template half<0>(w[1]);
  const uint32_t l0 = Op::template half<1>(w[1]), d0 = Op::template half<0>(w[2]), u0 = Op::template half<1>(w[2]), y0 = Op::template half<0>(w[3]);
  const uint32_t f0 = Op::template half<1>(w[3]), t0 = Op::template half<0>(w[4]);
  const uint32_t l1 = Op::template half<1>(w[4]), d1 = Op::template half<0>(w[5]), u1 = Op::template half<1>(w[5]), y1 = Op::template half<0>(w[6]);
  const uint32_t f1 = Op::template half<1>(w[6]), t1 = Op::template half<0>(w[7]);
  const bool two = (meta & 3u) == 2u, o0 = (meta >> 4) & 1u, o1 = (meta >> 5) & 1u;
  const bool new_aii = FRESH && (meta & SPICEY_ROW_FRESH_AII), new_t0 = FRESH && (meta & SPICEY_ROW_FRESH_O0), new_t1 = FRESH && (meta & SPICEY_ROW_FRESH_O1);
  for (int k = 0; k < K; k++) {
    // every operand in one LDS round trip (an unused second pivot / fill: index 0, a valid address; results masked)
    double aii = 0.0;
    if (!new_aii) aii = Op::template ld<K>(c.W, iaa, k);
    double yi = Op::template ld<K>(c.W, iy, k);
    const double vl0 = Op::template ld<K>(E, l0, k), vd0 = Op::template ld<K>(E, d0, k), vy0 = Op::template ld<K>(c.W, y0, k), vu0 = Op::template ld<K>(E, u0, k);
    const double vl1 = Op::template ld<K>(E, l1, k), vd1 = Op::template ld<K>(E, d1, k), vy1 = Op::template ld<K>(c.W, y1, k), vu1 = Op::template ld<K>(E, u1, k);
    const double vf0 = Op::template ld<K>(E, f0, k);
    double vt0 = 0.0, vt1 = 0.0;
    if (!new_t0) vt0 = Op::template ld<K>(c.W, t0, k);
    const double vf1 = Op::template ld<K>(E, f1, k);
    if (!new_t1) vt1 = Op::template ld<K>(c.W, t1, k);
    const double m0 = -(vl0 * vd0), m1 = -(vl1 * vd1);
    yi = fma(m0, vy0, yi);
    aii = fma(m0, vu0, aii);
    const double y2 = fma(m1, vy1, yi), a2 = fma(m1, vu1, aii);
    yi = two ? y2 : yi;
    aii = two ? a2 : aii;
    Op::template st<K>(c.W, iy, k, yi);
    if (!rhs_only) {
      if (o0) Op::template st<K>(c.W, t0, k, fma(m0, vf0, vt0));
      if (two && o1) Op::template st<K>(c.W, t1, k, fma(m1, vf1, vt1));
      if (meta & (SPICEY_R16_RECIP << 8)) {
        if (fabs(aii) < SPICEY_EPS && c.valid[k]) { c.flags[1] = 1; c.flags[2] = c.inst[k]; }
        aii = spicey_rcp(aii);
      }
      Op::template st<K>(c.W, iaa, k, aii);
    }
  }
}

// Two row records of the leaves' factor phase under the hybrid workspace (OPG): the global operands of BOTH are fetched first,
// then each record runs exactly as spicey_exec_row16 would (same products, same order: the rows of one level are independent).
template <int K>
SPICEY_HD void spicey_exec_row16_x2(const WgCtx<K> &c, const uint32_t *wa, const uint32_t *wb, bool rhs_only) {
  static_assert(K == 1, "hybrid workspace: one instance per workgroup");
  const uint32_t *w2[2] = {wa, wb};
  double gl[2][2], gdg[2][2], gu[2][2], gf[2][2];
  SPICEY_UNROLL
  for (int r = 0; r < 2; r++) {
    const uint32_t *w = w2[r];
    const uint32_t l0 = w[1] >> 16, d0 = w[2] & 0xffffu, u0 = w[2] >> 16, f0 = w[3] >> 16;
    const uint32_t l1 = w[4] >> 16, d1 = w[5] & 0xffffu, u1 = w[5] >> 16, f1 = w[6] >> 16;
    gl[r][0] = c.G[l0]; gdg[r][0] = c.G[d0]; gu[r][0] = c.G[u0]; gf[r][0] = c.G[f0];
    gl[r][1] = c.G[l1]; gdg[r][1] = c.G[d1]; gu[r][1] = c.G[u1]; gf[r][1] = c.G[f1];
  }
  SPICEY_UNROLL
  for (int r = 0; r < 2; r++) {
    const uint32_t *w = w2[r];
    const uint32_t meta = w[0] >> 16;
    if (!(meta & (SPICEY_R16_VALID << 8))) continue;
    const uint32_t iaa = w[0] & 0xffffu, iy = w[1] & 0xffffu;
    const uint32_t y0 = w[3] & 0xffffu, t0 = w[4] & 0xffffu, y1 = w[6] & 0xffffu, t1 = w[7] & 0xffffu;
    const bool two = (meta & 3u) == 2u, o0 = (meta >> 4) & 1u, o1 = (meta >> 5) & 1u;
    double aii = c.W[iaa], yi = c.W[iy];
    const double vy0 = c.W[y0], vy1 = c.W[y1], vt0 = c.W[t0], vt1 = c.W[t1];
    const double m0 = -(gl[r][0] * gdg[r][0]), m1 = -(gl[r][1] * gdg[r][1]);
    yi = fma(m0, vy0, yi);
    aii = fma(m0, gu[r][0], aii);
    const double y2 = fma(m1, vy1, yi), a2 = fma(m1, gu[r][1], aii);
    yi = two ? y2 : yi;
    aii = two ? a2 : aii;
    c.W[iy] = yi;
    if (!rhs_only) {
      if (o0) c.W[t0] = fma(m0, gf[r][0], vt0);
      if (two && o1) c.W[t1] = fma(m1, gf[r][1], vt1);
      if (meta & (SPICEY_R16_RECIP << 8)) {
        if (fabs(aii) < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
        aii = spicey_rcp(aii);
      }
      c.W[iaa] = aii;
    }
  }
}

// the phase table of this workgroup (`on`: wave-uniform, fixed for the run) and the row of the phase at hand
struct SpiceyPt {
  const uint32_t *w;
  bool on;
  int row;
};

// P, Q: the argument structs where they live (global memory on the GPU).  Nothing is fetched from them, or from the phase
// table, before it is needed: a resident phase of tasks with at most two products reads no argument at all.
// UR (the resident-record form of the fresh build, tran_v2_run.h): rr.u0 is not this function's — phase 0 runs
// spicey_u0_resident_phase instead, and the other factor phases leave the words alone.
template <int K, int RMAX, int NSV, int NEL, bool KTASK, bool OPG = false, bool OA = false, bool UR = false>
SPICEY_HD void spicey_uk_phase(const SpiceyProg &P, const SpiceyResident &Q, const SpiceyPt pt, const WgCtx<K> &c, ResRegs<K, RMAX, NSV, NEL> &rr, int tid,
                               int T, int p, bool streamed, bool reuse = false) {
  constexpr bool FRESH = SpiceyShapeKind<RMAX, NSV, NEL>::fresh;
  auto ovf = [&]() -> const uint16_t * { return pt.on ? spicey_pt_ptr<const uint16_t>(pt.w, SPICEY_PT_OVF16) : spicey_fresh(P).ovf16; };
  uint32_t xoff = 0u;  // first LDS index of the right-hand side (= nLU without the hybrid layout)
  if (OPG || (!KTASK && reuse)) xoff = pt.on ? spicey_pt_u32(pt.w, SPICEY_PT_XOFF) : (uint32_t)spicey_fresh(P).xoff;
  const uint32_t keep_from = (!KTASK && reuse) ? xoff : 0u;
  if (RMAX <= 8) {
    // few slots: a static compare chain (scalar compares on the wave-uniform phase bytes).  Measured faster than
    // both indexed register access and a binary decision tree on a slot cursor (11.8 vs 16.0 / 15.2 us per step).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < RMAX; s++) {
      const int sp = SPICEY_UNIFORM((int)((rr.phv[s >> 2] >> ((s & 3) * 8)) & 0xffu));
      if (sp == p) {
        uint32_t w0 = rr.w0[s], w1 = rr.w1[s], w2 = rr.w2[s], w3 = rr.w3[s];
        SPICEY_OPAQUE(w0); SPICEY_OPAQUE(w1); SPICEY_OPAQUE(w2); SPICEY_OPAQUE(w3);
        if (!KTASK && s + 1 < RMAX && SPICEY_UNIFORM((int)((rr.phv[(s + 1) >> 2] >> (((s + 1) & 3) * 8)) & 0xffu)) == 0xFE) {  // a chunk of row records: this slot + its continuation
          uint32_t w[8] = {w0, w1, w2, w3, rr.w0[s + 1 < RMAX ? s + 1 : s], rr.w1[s + 1 < RMAX ? s + 1 : s], rr.w2[s + 1 < RMAX ? s + 1 : s], rr.w3[s + 1 < RMAX ? s + 1 : s]};
          SPICEY_OPAQUE(w[4]); SPICEY_OPAQUE(w[5]); SPICEY_OPAQUE(w[6]); SPICEY_OPAQUE(w[7]);
          spicey_exec_row16<K, OPG, FRESH, OA>(c, w, reuse);
        } else {
          spicey_exec_rec16<K, KTASK, OPG, FRESH, OA>(c, ovf, w0, w1, w2, w3, keep_from, xoff);
        }
      }
    }
  } else {
    // resident chunks of this wave that belong to phase p: consecutive slots starting at the cursor;
    // the slot index is wave-uniform, the records are fetched through the VGPR index register
    int q = rr.cursor;
    while (q < RMAX) {
      const uint32_t pw = rr.phv[q >> 2];
      const int sp = SPICEY_UNIFORM((int)((pw >> ((q & 3) * 8)) & 0xffu));
      if (sp != p) break;
      uint32_t w0 = rr.w0[q], w1 = rr.w1[q], w2 = rr.w2[q], w3 = rr.w3[q];
      SPICEY_OPAQUE(w0); SPICEY_OPAQUE(w1); SPICEY_OPAQUE(w2); SPICEY_OPAQUE(w3);
      if (!KTASK && q + 1 < RMAX && SPICEY_UNIFORM((int)((rr.phv[(q + 1) >> 2] >> (((q + 1) & 3) * 8)) & 0xffu)) == 0xFE) {  // a chunk of row records: this slot + its continuation
        uint32_t w[8] = {w0, w1, w2, w3, rr.w0[q + 1], rr.w1[q + 1], rr.w2[q + 1], rr.w3[q + 1]};
        SPICEY_OPAQUE(w[4]); SPICEY_OPAQUE(w[5]); SPICEY_OPAQUE(w[6]); SPICEY_OPAQUE(w[7]);
        spicey_exec_row16<K, OPG, FRESH, OA>(c, w, reuse);
        q += 2;
      } else {
        spicey_exec_rec16<K, KTASK, OPG, FRESH, OA>(c, ovf, w0, w1, w2, w3, keep_from, xoff);
        q++;
      }
    }
    rr.cursor = q;
  }
  if (!streamed) {
    if (FRESH && !KTASK && !UR) for (int i = 0; i < 8; i++) rr.u0[FRESH ? i : 0] = 0u;
    return;
  }
  // one 32-byte descriptor says where the phase's records are (SpiceyResident::st_desc): from the phase table in LDS — one
  // round trip between the phase head and the first record fetch — or through the argument structs (three)
  uint32_t d_rows, d_first, d_cnt, d_rhs, d_rfirst, d_rcnt, d_rrhs;
  const uint32_t *rec16, *fus16;
  if (pt.on) {
    const SpiceyPtLanes d = SpiceyPtLanes::row(pt.w, tid, pt.row);  // (the whole wave is here: `streamed` is wave-uniform)
    d_rows = d.u32(0); d_first = d.u32(1); d_cnt = d.u32(2); d_rhs = d.u32(3); d_rfirst = d.u32(4); d_rcnt = d.u32(5); d_rrhs = d.u32(6);
    rec16 = d.template ptr<const uint32_t>(SPICEY_PT_REC16);
    fus16 = KTASK ? nullptr : d.template ptr<const uint32_t>(SPICEY_PT_FUS16);
  } else {
    const SpiceyResident Qf = spicey_fresh(Q);
    const SpiceyProg Pf = spicey_fresh(P);
    const uint32_t *dsc = Qf.st_desc + (size_t)p * 8;
    d_rows = dsc[0]; d_first = dsc[1]; d_cnt = dsc[2]; d_rhs = dsc[3]; d_rfirst = dsc[4]; d_rcnt = dsc[5]; d_rrhs = dsc[6];
    rec16 = Pf.rec16;
    fus16 = Pf.fus16;
  }
  uint32_t sc = (!KTASK && reuse) ? d_rhs : d_cnt;  // right-hand-side tasks lead every factor phase
  const uint32_t *base = rec16 + (size_t)d_first * 4;
  if (!KTASK && sc && d_rows) {
    // the phase's row-record encoding: its 32-byte row records (one per thread on the chains this is for), then the few
    // generic records of rows that do not fit the pattern
    const uint32_t npair = d_cnt;
    const uint32_t *pb = fus16 + (size_t)d_first * 4;
    if constexpr (OPG && NEL >= 2) {
      // (hybrid workspace: the leaves' own entries come from L2 — two row records at a time, both fetched before either is
      // executed, so that the operand loads of the second are in flight under the first; the 1024-thread build — NEL = 1 —
      // has half the records per thread and no registers for a second one)
      SPICEY_NOUNROLL
      for (uint32_t j = (uint32_t)tid; j < npair; j += 2u * (uint32_t)T) {
        const uint32_t j2 = j + (uint32_t)T;
        const bool two = j2 < npair;
        uint32_t wa[8], wb[8];
        for (int i = 0; i < 8; i++) { wa[i] = pb[(size_t)j * 8 + i]; wb[i] = pb[(size_t)(two ? j2 : j) * 8 + i]; }
        if (!two) wb[0] = 0u;  // (no VALID flag: nothing runs)
        spicey_exec_row16_x2<K>(c, wa, wb, reuse);
      }
    } else
    SPICEY_NOUNROLL
    for (uint32_t j = (uint32_t)tid; j < npair; j += (uint32_t)T) {
      uint32_t w[8];
      // (fresh build, phase 0: record `tid` has been in flight since phase B — TranPhases2::u0_fetch, same address — a
      // run-time test, not a second copy of the phase body: profiles/NOTES_r05.md §6)
      if (FRESH && p == 0 && j == (uint32_t)tid) for (int i = 0; i < 8; i++) w[i] = rr.u0[FRESH ? i : 0];
      else for (int i = 0; i < 8; i++) w[i] = pb[(size_t)j * 8 + i];
      spicey_exec_row16<K, OPG, FRESH, OA>(c, w, reuse);
    }
    base = fus16 + (size_t)d_rfirst * 4;
    sc = reuse ? d_rrhs : d_rcnt;
  }
  if (sc) {
    // streamed phase (did not fit the resident slots): double-buffered — the next record's L2 fetch is in flight
    // while the current task executes.  (Fetching 4 records up front was measured slower: +16 live VGPRs pushed
    // the 1024-thread kernel to its 128-register cap.)
    uint32_t j = (uint32_t)tid;
    if (j < sc) {
      const uint32_t *r = base + (size_t)j * 4;
      uint32_t c0 = r[0], c1 = r[1], c2 = r[2], c3 = r[3];
      for (;;) {
        const uint32_t jn = j + (uint32_t)T;
        const bool more = jn < sc;
        const uint32_t *rn = base + (size_t)(more ? jn : j) * 4;
        const uint32_t n0 = rn[0], n1 = rn[1], n2 = rn[2], n3 = rn[3];
        spicey_exec_rec16<K, KTASK, OPG, FRESH, OA>(c, ovf, c0, c1, c2, c3, keep_from, xoff);
        if (!more) break;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        j = jn;
      }
    }
  }
  if (FRESH && !KTASK && !UR) for (int i = 0; i < 8; i++) rr.u0[FRESH ? i : 0] = 0u;  // (consumed, or not for this phase: dead until the next B)
}

// FS (the fixed-schedule build, tran_v2_run.h): a phase of a run in which every phase but level 0 is resident and no resident
// record has more than two products — the slot compare chain of spicey_uk_phase and nothing else.  No streamed tail, no
// descriptor, no phase-table read; no reused factorisation, so no `xoff`, `keep_from` or right-hand-side-only row; rr.u0 is
// the resident level-0 record's and stays; no overflow list.  The records run through the same executors with those
// arguments as constants: the arithmetic and its order are spicey_uk_phase's.
template <int K, int RMAX, int NSV, int NEL, bool KTASK, bool OA>
SPICEY_HD void spicey_uk_phase_fs(const WgCtx<K> &c, ResRegs<K, RMAX, NSV, NEL> &rr, int p) {
  static_assert(RMAX <= 8, "the fixed schedule is a form of the packed build: a static compare chain over its few slots");
  constexpr bool FRESH = SpiceyShapeKind<RMAX, NSV, NEL>::fresh;
  auto ovf = []() -> const uint16_t * { return nullptr; };  // (never asked: INL)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int s = 0; s < RMAX; s++) {
    const int sp = SPICEY_UNIFORM((int)((rr.phv[s >> 2] >> ((s & 3) * 8)) & 0xffu));
    if (sp == p) {
      uint32_t w0 = rr.w0[s], w1 = rr.w1[s], w2 = rr.w2[s], w3 = rr.w3[s];
      SPICEY_OPAQUE(w0); SPICEY_OPAQUE(w1); SPICEY_OPAQUE(w2); SPICEY_OPAQUE(w3);
      if (!KTASK && s + 1 < RMAX && SPICEY_UNIFORM((int)((rr.phv[(s + 1) >> 2] >> (((s + 1) & 3) * 8)) & 0xffu)) == 0xFE) {  // a chunk of row records: this slot + its continuation
        uint32_t w[8] = {w0, w1, w2, w3, rr.w0[s + 1 < RMAX ? s + 1 : s], rr.w1[s + 1 < RMAX ? s + 1 : s], rr.w2[s + 1 < RMAX ? s + 1 : s], rr.w3[s + 1 < RMAX ? s + 1 : s]};
        SPICEY_OPAQUE(w[4]); SPICEY_OPAQUE(w[5]); SPICEY_OPAQUE(w[6]); SPICEY_OPAQUE(w[7]);
        spicey_exec_row16<K, false, FRESH, OA>(c, w, false);
      } else {
        spicey_exec_rec16<K, KTASK, false, FRESH, OA, true>(c, ovf, w0, w1, w2, w3, 0u, 0u);
      }
    }
  }
}

// UR: factor phase 0 of a run whose level 0 is nothing but row records, at most one per thread (the host has made sure:
// launch_plan.h, spicey_plan_u0_resident) — the record has been in rr.u0 since the prologue.  No table row, no descriptor,
// no loop and no streamed path; the same record through the same spicey_exec_row16 as the streamed phase runs it, so the
// same bits.  The words are made opaque here like the resident slots', so that nothing decoded from them is kept around
// the time loop.  (Such a run never reuses a factorisation: rhs_only = false.)
template <int K, int RMAX, int NSV, int NEL, bool OA = false>
SPICEY_HD void spicey_u0_resident_phase(const WgCtx<K> &c, ResRegs<K, RMAX, NSV, NEL> &rr) {
  constexpr bool FRESH = SpiceyShapeKind<RMAX, NSV, NEL>::fresh;
  static_assert(FRESH, "the resident level-0 record is a form of the fresh build");
  uint32_t w[8];
  for (int i = 0; i < 8; i++) { w[i] = rr.u0[FRESH ? i : 0]; SPICEY_OPAQUE(w[i]); }
  spicey_exec_row16<K, false, FRESH, OA>(c, w, false);
}
