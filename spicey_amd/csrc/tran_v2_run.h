// tran_v2_run.h — the tridiagonal top and the v2 run driver, spicey_tran_run_v2 (tran_exec.h is the map).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "program.h"
#include "tran_common.h"
#include "tran_pt.h"
#include "tran_rec16.h"
#include "tran_v1_phases.h"
#include "tran_v2_phases.h"

// ---- tridiagonal top by parallel cyclic reduction (program.h: pcr_n, pcr_tab) -------------------------------------------
// One wave, lane i = row i of the tridiagonal Schur complement (path order), two SoA buffers {a, b, c, d}[64] in LDS used
// alternately.  Stage 0 gathers the rows from W through the index table; stage st = 1 .. S (stride 1, 2, 4, ...): row i
// eliminates its couplings to the rows i -+ stride with those rows' equations; after S = ceil(log2 n) stages every row
// stands alone and the last stage writes x_i = d_i / b_i straight into the solution slot.
// Replaces 2 x (S + 1) LDS-serial levels of the task lists; no U entries are formed for these pivots (nothing below needs
// them: the backward records of lower rows read x only).  All loads of a stage are unconditional (clamped addresses, values
// masked afterwards) so that they are issued together: one LDS round trip per stage.
template <int K>
SPICEY_HD void spicey_pcr_row(const WgCtx<K> &c, const uint16_t *tab, int n, int r, double &a, double &b, double &cc, double &d) {
  const bool on = r >= 0 && r < n;
  const int rr = on ? r : 0;
  const uint32_t ia = tab[rr * 4], ib = tab[rr * 4 + 1], ic = tab[rr * 4 + 2], id = tab[rr * 4 + 3];
  const double va = c.W[(size_t)(ia == 0xFFFFu ? ib : ia) * K], vb = c.W[(size_t)ib * K], vc = c.W[(size_t)(ic == 0xFFFFu ? ib : ic) * K],
               vd = c.W[(size_t)id * K];
  a = (on && ia != 0xFFFFu) ? va : 0.0;
  b = on ? vb : 1.0;  // rows past the end: identity
  cc = (on && ic != 0xFFFFu) ? vc : 0.0;
  d = on ? vd : 0.0;
}
// A row without a neighbour at the stage's stride has a zero coupling on that side (a_i = 0 for i < stride, c_i = 0 for
// i + stride >= n: by induction over the stages; rows past the end are identity rows), so the missing neighbour is not
// masked: its index is clamped into the buffer and whatever finite row is read there is multiplied by that zero.  (Masking
// cost 16 selects of ~70 instructions per stage, on a wave that issues one instruction per ~4.5 cycles.)
template <int K>
SPICEY_HD void spicey_pcr_stage(const WgCtx<K> &c, double *buf, const uint16_t *tab, int n, int S, int lane, int st, double *own) {
  // LDS row = {a, 1/b, c, d}: a row forms the reciprocal of its own pivot once, its two neighbours multiply with it;
  // the row's own {a, b, c, d} stay in registers (`own`) from stage to stage
  double *wr = buf + ((st & 1) ? 256 : 0);
  bool sing;
  if (st == 0) {  // gather the rows from W (stage 0 writes buffer 0)
    double a, b, cc, d;
    spicey_pcr_row<K>(c, tab, n, lane, a, b, cc, d);
    own[0] = a; own[1] = b; own[2] = cc; own[3] = d;
    sing = fabs(b) < SPICEY_EPS;
    wr[lane] = a; wr[64 + lane] = spicey_rcp(b); wr[128 + lane] = cc; wr[192 + lane] = d;
  } else {
    const double *rd = buf + (((st - 1) & 1) ? 256 : 0);
    const int h = 1 << (st - 1), im = lane - h, ip = lane + h;
    const int jm = im < 0 ? 0 : im, jp = ip > 63 ? 63 : ip;
    const double am = rd[jm], rm = rd[64 + jm], cm = rd[128 + jm], dm = rd[192 + jm];
    const double ap = rd[jp], rp = rd[64 + jp], cp = rd[128 + jp], dp = rd[192 + jp];
    const double al = -own[0] * rm;  // (a = 0 where there is no such neighbour)
    const double ga = -own[2] * rp;
    const double na = al * am, nc = ga * cp;
    const double nb = fma(ga, ap, fma(al, cm, own[1]));
    const double nd = fma(ga, dp, fma(al, dm, own[3]));
    sing = fabs(nb) < SPICEY_EPS;
    const double nr = spicey_rcp(nb);
    if (st < S) {
      own[0] = na; own[1] = nb; own[2] = nc; own[3] = nd;
      wr[lane] = na; wr[64 + lane] = nr; wr[128 + lane] = nc; wr[192 + lane] = nd;
    } else if (lane < n) {  // the rows are decoupled: x = d / b straight into the solution slot
      c.W[(size_t)tab[lane * 4 + 3] * K] = nd * nr;
    }
  }
  if (sing && lane < n && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
}
// TF (the fold of the last factor level into the top, a form of the resident-record build): on the packed chains the factor
// level right below the top is nothing but row records whose targets ARE the top's rows — a_ii, y_i and the two fills toward
// the neighbouring top rows.  As a phase it wrote the four values into W, met the workgroup at a barrier, and the top's lane
// read the same four back as {b, d, a, c}.  Here lane i runs row i's record itself, at the head of the top, and keeps the
// results: no phase, no barrier, no round trip, and nothing of the row reaches W but x.  The record comes from a table the
// host has built (launch_plan.h: spicey_top_fold_table — its conditions are stated there) and the prologue has copied into
// the top's first row buffer, which the register-exchange top leaves unused: every target of the program's row record has
// become a read operand (a created entry reads the +0.0 slot, a side without a fill the entry as it stands), so the 14
// operands are read unconditionally, in one round trip.  The arithmetic is spicey_exec_row16's, operation for operation:
// m = -(l d), y = fma(m0, y0, y), a_ii = fma(m0, u0, a_ii), the second pivot under `two`, the fills fma(m, f, t).
// none_a / none_c: the row has no neighbour on that side (pcr_tab: 0xFFFF); on: the lane holds a row of the top.
template <int K, bool OA>
SPICEY_HD void spicey_top_fold_row(const WgCtx<K> &c, const uint32_t *w, bool none_a, bool none_c, bool on, double &a, double &b, double &cc, double &d) {
  static_assert(K == 1, "the fold is a form of the register-exchange top: one instance per workgroup");
  typedef SpiceyOperand<OA> Op;
  const uint32_t meta = w[0] >> 16;
  const uint32_t iaa = Op::template half<0>(w[0]), iy = Op::template half<0>(w[1]);
  const uint32_t l0 = Op::template half<1>(w[1]), d0 = Op::template half<0>(w[2]), u0 = Op::template half<1>(w[2]), y0 = Op::template half<0>(w[3]);
  const uint32_t f0 = Op::template half<1>(w[3]), t0 = Op::template half<0>(w[4]);
  const uint32_t l1 = Op::template half<1>(w[4]), d1 = Op::template half<0>(w[5]), u1 = Op::template half<1>(w[5]), y1 = Op::template half<0>(w[6]);
  const uint32_t f1 = Op::template half<1>(w[6]), t1 = Op::template half<0>(w[7]);
  const bool one = (meta & 3u) != 0u, two = (meta & 3u) == 2u, o0 = (meta >> 4) & 1u, o1 = (meta >> 5) & 1u, side = (w[7] >> 16) & 1u;
  double aii = Op::template ld<K>(c.W, iaa, 0), yi = Op::template ld<K>(c.W, iy, 0);
  const double vl0 = Op::template ld<K>(c.W, l0, 0), vd0 = Op::template ld<K>(c.W, d0, 0), vy0 = Op::template ld<K>(c.W, y0, 0), vu0 = Op::template ld<K>(c.W, u0, 0);
  const double vl1 = Op::template ld<K>(c.W, l1, 0), vd1 = Op::template ld<K>(c.W, d1, 0), vy1 = Op::template ld<K>(c.W, y1, 0), vu1 = Op::template ld<K>(c.W, u1, 0);
  const double vf0 = Op::template ld<K>(c.W, f0, 0), vt0 = Op::template ld<K>(c.W, t0, 0), vf1 = Op::template ld<K>(c.W, f1, 0), vt1 = Op::template ld<K>(c.W, t1, 0);
  const double m0 = -(vl0 * vd0), m1 = -(vl1 * vd1);
  const double ya = fma(m0, vy0, yi), aa = fma(m0, vu0, aii);
  yi = one ? ya : yi;  // (a row without a record: its entries as they stand)
  aii = one ? aa : aii;
  const double y2 = fma(m1, vy1, yi), a2 = fma(m1, vu1, aii);
  yi = two ? y2 : yi;
  aii = two ? a2 : aii;
  const double g0 = fma(m0, vf0, vt0), g1 = fma(m1, vf1, vt1);
  const double e0 = (one && o0) ? g0 : vt0, e1 = (two && o1) ? g1 : vt1;
  const double sub = side ? e1 : e0, sup = side ? e0 : e1;
  a = (on && !none_a) ? sub : 0.0;
  b = on ? aii : 1.0;  // rows past the end: identity
  cc = (on && !none_c) ? sup : 0.0;
  d = on ? yi : 0.0;
}
// The folded top of one wave as the host runs it: "record, then the stages" with the lane exchange of spicey_pcr_all_regs
// as array indexing — the same operations in the same order, the same clamped neighbours, the pivots judged by their
// running minimum.  `rec`: the 64 records of the table, `tab`: the top's index table.  Writes x and nothing else.
template <int K>
SPICEY_HD void spicey_top_fold_wave(const WgCtx<K> &c, const uint32_t *rec, const uint16_t *tab, int n, int S) {
  double a[64], b[64], cc[64], d[64], r[64], pmin[64];
  for (int lane = 0; lane < 64; lane++) {
    const bool on = lane < n;
    const uint16_t *t = tab + (on ? lane : 0) * 4;
    spicey_top_fold_row<K, false>(c, rec + (size_t)lane * 8, t[0] == 0xFFFFu, t[2] == 0xFFFFu, on, a[lane], b[lane], cc[lane], d[lane]);
    pmin[lane] = fabs(b[lane]);
    r[lane] = spicey_rcp(b[lane]);
  }
  for (int st = 1; st <= S; st++) {
    const int h = 1 << (st - 1);
    double na[64], nb[64], nc[64], nd[64], nr[64];
    for (int lane = 0; lane < 64; lane++) {
      const int jm = lane - h < 0 ? 0 : lane - h, jp = lane + h > 63 ? 63 : lane + h;
      const double al = -a[lane] * r[jm], ga = -cc[lane] * r[jp];
      na[lane] = st < S ? al * a[jm] : 0.0;  // (dead in the last stage)
      nc[lane] = st < S ? ga * cc[jp] : 0.0;
      nb[lane] = fma(ga, a[jp], fma(al, cc[jm], b[lane]));
      nd[lane] = fma(ga, d[jp], fma(al, d[jm], d[lane]));
      pmin[lane] = fmin(pmin[lane], fabs(nb[lane]));
      nr[lane] = spicey_rcp(nb[lane]);
    }
    for (int lane = 0; lane < 64; lane++) {
      if (st < S) { a[lane] = na[lane]; b[lane] = nb[lane]; cc[lane] = nc[lane]; d[lane] = nd[lane]; r[lane] = nr[lane]; }
      else if (lane < n) c.W[(size_t)tab[lane * 4 + 3] * K] = nd[lane] * nr[lane];
    }
  }
  for (int lane = 0; lane < n && lane < 64; lane++)
    if (pmin[lane] < SPICEY_EPS && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
}
#if defined(__HIP_DEVICE_COMPILE__)
// All stages in one call for the GPU (the same arithmetic as spicey_pcr_stage, stage after stage): the stage loop is
// unrolled — strides, buffer halves and the last-stage test are constants —, the pivots are judged once at the end by
// their running minimum, and between two stages stands only a compiler fence (the LDS operations of one wave execute in
// order).  ~40 instructions per stage instead of ~70.
template <int K>
__device__ __forceinline__ void spicey_pcr_all(const WgCtx<K> &c, double *buf, const uint16_t *tab, int n, int S, int lane) {
  double a, b, cc, d;
  spicey_pcr_row<K>(c, tab, n, lane, a, b, cc, d);
  double pmin = fabs(b);  // (rows past the end: b = 1)
  buf[lane] = a; buf[64 + lane] = spicey_rcp(b); buf[128 + lane] = cc; buf[192 + lane] = d;
#pragma unroll
  for (int st = 1; st <= 6; st++) {
    if (st > S) break;  // (wave-uniform)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const double *rd = buf + (((st - 1) & 1) ? 256 : 0);
    double *wr = buf + ((st & 1) ? 256 : 0);
    const int h = 1 << (st - 1);
    const int jm = max(lane - h, 0), jp = min(lane + h, 63);
    const double am = rd[jm], rm = rd[64 + jm], cm = rd[128 + jm], dm = rd[192 + jm];
    const double ap = rd[jp], rp = rd[64 + jp], cp = rd[128 + jp], dp = rd[192 + jp];
    const double al = -a * rm, ga = -cc * rp;
    const double na = al * am, nc = ga * cp;
    const double nb = fma(ga, ap, fma(al, cm, b));
    const double nd = fma(ga, dp, fma(al, dm, d));
    pmin = fmin(pmin, fabs(nb));
    const double nr = spicey_rcp(nb);
    if (st < S) {
      a = na; b = nb; cc = nc; d = nd;
      wr[lane] = na; wr[64 + lane] = nr; wr[128 + lane] = nc; wr[192 + lane] = nd;
    } else if (lane < n) {
      c.W[(size_t)tab[lane * 4 + 3] * K] = nd * nr;
    }
  }
  if (pmin < SPICEY_EPS && lane < n && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
}
// TR (the register-exchange top, a form of the operand-address build): the same stages with the rows in registers.  A row
// keeps {a, b, c, d} and r = 1/b from stage to stage and reads {a, r, c, d} of the rows lane -+ stride from those lanes'
// registers (ds_bpermute on the halves of each double: the LDS crossbar, no LDS memory), so a stage holds no ds_write, no
// wait for it and no fence — values that only ever move between the lanes of one wave no longer make the round trip
// through LDS.  The arithmetic is spicey_pcr_all's, operation for operation, and so is the clamped-neighbour rule: lane 0 /
// lane 63 stand in for a missing neighbour and their finite row is multiplied by the same zero coupling.
// Condition: ALL 64 lanes of the wave execute this (ds_bpermute returns 0 for a lane that does not) — wave 0 of
// gpu_wave_lockstep_keep_then with nlanes = 64, which is how spicey_tran_run_v2 calls it; rows past n are identity rows in
// their lanes' registers as they were in the buffers.  The two row buffers stay allocated (the LDS layout is every
// build's) and unused.  The gather reads the lane's four 16-bit indices as one 8-byte word pair and forms the operand
// addresses with the OA handles (c.W is LDS address 0); 0xFFFF, "no neighbour", is tested on the handle.
static __device__ __forceinline__ double spicey_lane_f64(int byte_lane, double v) {
  const int lo = __builtin_amdgcn_ds_bpermute(byte_lane, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(byte_lane, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// TF (above): the head runs the lane's fold record — read together with the index entry, which still says where x goes and
// which neighbours exist — instead of gathering the row from W; and the last stage, whose na and nc are dead, issues no
// exchange for them (the compiler does not sink the four ds_bpermute into the branch by itself).
template <int K, bool TF = false>
__device__ __forceinline__ void spicey_pcr_all_regs(const WgCtx<K> &c, const uint16_t *tab, int n, int S, int lane) {
  static_assert(K == 1, "the register-exchange top is a form of the operand-address build");
  typedef SpiceyOperand<true> Op;
  const bool on = lane < n;
  const uint2 t = *(const uint2 *)(tab + (on ? lane : 0) * 4);  // {ia | ib << 16, ic | id << 16}: 8-byte aligned
  const uint32_t none = Op::index(0xFFFFu);
  const uint32_t ha = Op::template half<0>(t.x), hb = Op::template half<1>(t.x), hc = Op::template half<0>(t.y), hd = Op::template half<1>(t.y);
  double a, b, cc, d;
  if constexpr (TF) {
    const uint4 r0 = *(const uint4 *)(c.tail + lane * 8), r1 = *(const uint4 *)(c.tail + lane * 8 + 4);  // (64 records: a lane past n holds zeros)
    const uint32_t w[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    spicey_top_fold_row<K, true>(c, w, ha == none, hc == none, on, a, b, cc, d);
  } else {
    const double va = Op::template ld<K>(c.W, ha == none ? hb : ha, 0), vb = Op::template ld<K>(c.W, hb, 0), vc = Op::template ld<K>(c.W, hc == none ? hb : hc, 0),
                 vd = Op::template ld<K>(c.W, hd, 0);
    a = (on && ha != none) ? va : 0.0;
    b = on ? vb : 1.0;  // rows past the end: identity
    cc = (on && hc != none) ? vc : 0.0;
    d = on ? vd : 0.0;
  }
  double pmin = fabs(b);
  double r = spicey_rcp(b);
#pragma unroll
  for (int st = 1; st <= 6; st++) {
    if (st > S) break;  // (wave-uniform)
    const int h = 1 << (st - 1);
    const int jm = max(lane - h, 0) << 2, jp = min(lane + h, 63) << 2;
    // (the operands of the pivot chain first)
    const double rm = spicey_lane_f64(jm, r), cm = spicey_lane_f64(jm, cc), rp = spicey_lane_f64(jp, r), ap = spicey_lane_f64(jp, a);
    const double dm = spicey_lane_f64(jm, d), dp = spicey_lane_f64(jp, d);
    double am = 0.0, cp = 0.0;
    if (!TF || st < S) { am = spicey_lane_f64(jm, a); cp = spicey_lane_f64(jp, cc); }  // (wave-uniform: all 64 lanes exchange, or none)
    const double al = -a * rm, ga = -cc * rp;
    const double na = al * am, nc = ga * cp;
    const double nb = fma(ga, ap, fma(al, cm, b));
    const double nd = fma(ga, dp, fma(al, dm, d));
    pmin = fmin(pmin, fabs(nb));
    const double nr = spicey_rcp(nb);
    if (st < S) {
      a = na; b = nb; cc = nc; d = nd; r = nr;
    } else if (on) {
      Op::template st<K>(c.W, hd, 0, nd * nr);
    }
  }
  if (pmin < SPICEY_EPS && on && c.valid[0]) { c.flags[1] = 1; c.flags[2] = c.inst[0]; }
}
#endif

// The three argument structs hold ~110 pointers: kept in SGPRs across the time loop they overflow the 102 scalar registers
// of a wave and the compiler parks them in VGPR lanes (round 1: 274 spilled SGPRs, 1 209 v_readlane in the kernel — 13 % of
// its instructions).  No phase of the time loop therefore sees the structs themselves.  Where the run keeps a phase table
// (tran_pt.h) a phase reads the words it needs from LDS; otherwise, and in the rarely taken branches, it takes the
// structs through `ex.fresh()` / spicey_fresh(): on the GPU they live in global memory and `fresh` makes their address
// opaque for this phase, so the fields it needs are fetched by scalar loads inside it (scalar cache).  Either way the
// values are dead at the phase's barrier; only a handful of loop-control scalars stay live around the loop.
// EP (the early-prefetch build, TranPhases2): every thread issues the loads of Z's parameter record, and thread(s) tid < nV
// that of the next step's source value, between the factor and the backward phases instead of at the tail of the last
// backward one; the last backward phase parks the source value in LDS, Z reads registers that arrived long ago, and B
// holds no global load of its own but phase 0's record.  R.zpar is not null in such a build.  Where the fetch stands:
//   - an executor with `idle_waves` (SpiceyHasIdleWaves: the GPU's) runs it in the phase of the tridiagonal top, through
//     wave_lockstep_keep_then: the waves that have no part in the top issue it at once and wait at the barrier, the top's
//     wave issues it behind the top — so the 22 registers are never live beside the top's own ~50.  (At the tail of the
//     last factor phase they are, and the packed build then spills 20 of them.  Moving the top wave's share to the head
//     of the next backward phase was measured too: that phase grew by what the top's had, ~500 cycles, and the headline
//     fell below the parent's.)  A program without a top gets a phase of its own for it.
//   - any other executor peels the last factor phase below the top — or the last of all — and fetches at its tail.
// Either way the fetch is unconditional code on every path through the iteration, so the registers are not live around
// the time loop.
template <class E, class = void>
struct SpiceyHasIdleWaves { static constexpr bool value = false; };
template <class E>
struct SpiceyHasIdleWaves<E, decltype((void)E::idle_waves)> { static constexpr bool value = true; };
// OS (the operand-slot build, TranPhases2): an early-prefetch build whose prologue writes the two constants of the operand
// slots (tran_pt_layout.h), resolves ground in Z's resident terminal indices to the +0.0 slot and the empty fields of B's
// resident descriptors to the -0.0 slot, and keeps the instance's row bases in the phase table; the caller has made sure
// that spicey_slots_fit holds for the program (the launch plan; it implies a phase table, whose free tail the slots take).
// RA (the ready-argument build, TranPhases2): an operand-slot build whose prologue also makes the table's record, source and
// iteration-count pointers this instance's own (spicey_pt_rebase_ready), whose Z and early fetch move only their hot
// arguments to scalars (spicey_pt_args_z / spicey_pt_args_early; the last-step test comes from `steps` below) and read the
// rest inside the branch that needs it; the caller has made sure that spicey_ready_steps_ok holds for the run.
// OA (the operand-address build, TranPhases2 / tran_common.h: SpiceyOperand): a ready-argument build that names the operands
// of its always-executed LDS reads and writes — the interpreter's inline tasks and row records, Z's and B's resident
// sections — by handles; the caller has made sure that c.W is LDS address 0 and that spicey_addr_fits holds.
// TR (the register-exchange top, spicey_pcr_all_regs above): an operand-address build on the GPU whose unrolled top keeps
// its rows in registers; the caller has made sure that the top has 1 .. 6 stages (a top outside that range runs the staged
// form here as in every build).  Host executors run spicey_pcr_stage whatever TR says.
// UR (the resident level-0 record, a form of the register-exchange-top build of the fresh shape): factor level 0 of the
// packed chains is the one streamed phase of this shape, and its record — one 32-byte row record per thread — is the same
// in every step.  The prologue loads it once (TranPhases2::load_resident), B fetches nothing, phase 0 executes the
// registers (spicey_u0_resident_phase: no table row, no loop, no streamed path) and no factor phase clears them or waits
// for a fetch.  The caller has made sure that phase 0 is streamed in its row-record encoding, has at most T row records
// and no generic remainder, and that the run never reuses a factorisation (launch_plan.h: spicey_plan_u0_resident).
// TF (the fold of the last factor level into the top, spicey_top_fold_row above; a form of the resident-record build): the
// prologue copies the record table (behind R.zpar: program.h) into the top's first row buffer, the loop over the factor phases leaves phase pcr_level - 1
// out — no phase, no barrier; its records stay in their slots and are never dispatched — and the top's head runs the row's
// record.  The caller has made sure that spicey_top_fold_table holds for the program (launch_plan.h: spicey_plan_top_fold).
// A host executor runs the whole folded top in one call (spicey_top_fold_wave) where the GPU runs spicey_pcr_all_regs.
// SF (the stamp fuse, TranPhases2; a form of the folded build): the time loop holds no phase B.  The prologue stamps step 0
// with today's B, once, behind a0_initial's barrier, and then re-deals the descriptor registers from the host's table
// (behind the fold's, behind R.zpar: tran_pt_layout.h); a pivot below SPICEY_EPS found there ends the run as step 0's B would
// have ended it — code 1 at step 0, iteration 0, nothing recorded.  Z is two phases with one barrier between them: the first
// is Z with the stamp arithmetic and writes the matrix entries, which have no reader between K_0's barrier and U_0; the
// second writes the next right-hand side over the solution once every reader of it has read (a row's slot holds x_r until
// then, and its readers sit in other waves) — three stores from registers and nothing else.  The
// caller has made sure that spicey_stamp_fuse_table holds for the program (launch_plan.h: spicey_plan_stamp_fuse): no
// switch — the loop below never re-iterates —, nothing beyond the resident capacity, not linear.
// FS (the fixed schedule, a form of the fused build): the plan has decided, for the whole run, what the loop of every other
// form decides again in every phase of every step — which phases exist and are resident, that the table is on, that nothing
// re-iterates, that Z's parameters were fetched early — and the time loop is written out for it: U_0 from the resident
// record, the resident factor levels 1 .. pcr_level - 2 (spicey_uk_phase_fs), the folded top with the merged backward phase
// and the early fetch, the remaining backward phases, the last with the source park, Z, the second phase of Z.  No iteration
// loop, no S, A or diagnostics phase, no phase masks, no fork on the table; issue priorities are constants of each call
// (an executor with `fixed_priority`: phase_at) and an executor built without profiling holds no timer code.  The iteration
// counts — always 1 — are written once, behind the loop, for the steps that were recorded.  The caller has made sure that
// spicey_fixed_schedule_fits holds for the program and its resident layout (launch_plan.h: spicey_plan_fixed_schedule).
template <class E, class = void>
struct SpiceyHasFixedPriority { static constexpr bool value = false; };
template <class E>
struct SpiceyHasFixedPriority<E, decltype((void)E::fixed_priority)> { static constexpr bool value = true; };
// a phase whose issue priority `PR` (0 = none) is a constant of the call; executors without priorities run a plain phase
template <int PR, class Exec, class F>
SPICEY_HD void spicey_phase_at(Exec &ex, int tag, F f) {
  if constexpr (SpiceyHasFixedPriority<Exec>::value) ex.template phase_at<PR>(tag, f);
  else ex.phase(tag, f);
}
template <int K, int RMAX, int NSV, int NEL, bool HYB = false, int PT = -1, bool EP = false, bool OS = false, bool RA = false, bool OA = false, bool TR = false, bool UR = false, bool TF = false, bool SF = false, bool FS = false, class Exec>
SPICEY_HD void spicey_tran_run_v2(Exec &ex, const SpiceyProg &P, const SpiceyResident &Q, const SpiceyRun &R, WgCtx<K> &c, int wg) {
  static_assert(!FS || (SF && K == 1 && !HYB), "the fixed schedule is a form of the fused build");
  const int T = ex.threads();
  static_assert(!OS || PT != 0, "the operand slots lie behind the phase table");
  static_assert(!RA || OS, "the ready arguments are a form of the operand-slot build");
  static_assert(!OA || RA, "the operand addresses are a form of the ready-argument build");
  static_assert(!TR || (OA && K == 1), "the register-exchange top is a form of the operand-address build");
  static_assert(!UR || (TR && !HYB && SpiceyShapeKind<RMAX, NSV, NEL>::fresh), "the resident level-0 record is a form of the register-exchange-top build of the fresh shape");
  static_assert(!TF || UR, "the fold of the last factor level is a form of the resident-record build");
  static_assert(!SF || (TF && PT != 0), "the stamp fuse is a form of the folded build");
  typedef TranPhases2<K, RMAX, NSV, NEL, HYB, EP, OS, RA, OA, SF> Ph2;
  uint32_t brem, zrem;
  {
    Ph2 p2{P, R, c, T, 0u, 0u};
    p2.set_remainders();
    brem = p2.brem; zrem = p2.zrem;
  }
  typedef ResRegs<K, RMAX, NSV, NEL> Regs;
  // the phase table: tridiagonal-top builds whose rows fit behind the top's index table (wave-uniform, fixed for the run)
  static_assert(PT <= 0 || K == 1, "the phase table is built for one instance per workgroup");
  const bool pt_run = PT >= 0 ? PT == 1 : (K == 1 && spicey_pt_runtime_choice(P, Q));
  if (pt_run) ex.phase(SPICEY_PH_PRO, [&](int tid) { spicey_pt_build<K>(P, Q, R, c, tid, T, EP); if (OS) spicey_pt_rebase_rows<K>(P, R, c, tid); if (RA) spicey_pt_rebase_ready<K>(P, R, c, tid, (size_t)NEL * (size_t)T * 5); });  // (the structs where they live: see there)
  ex.phase(SPICEY_PH_PRO, [&](int tid) {
    const SpiceyProg Pf = ex.fresh(P); const SpiceyResident Qf = ex.fresh(Q); const SpiceyRun Rf = ex.fresh(R);
    TranPhases<K> ph{Pf, Rf, c, T};
    Ph2 p2{Pf, Rf, c, T, brem, zrem};
    if (tid == 0) { c.flags[0] = 0; c.flags[1] = 0; c.flags[2] = -1; }
    ph.p0_gstat(tid);
    p2.template load_resident<UR>(tid, Qf, ex.template regs<Regs>(tid));
    if (K == 1 && Pf.pcr_n > 0) {  // tridiagonal top: its index table sits behind the two 2 KB row buffers
      uint16_t *tab = (uint16_t *)(c.tail + 1024);
      for (int i = tid; i < Pf.pcr_n * 4; i += T) tab[i] = Pf.pcr_tab[i];
      if constexpr (TF) {  // the fold's records: the first row buffer, unused by the register-exchange top
        const uint32_t *fold = (const uint32_t *)(Rf.zpar + spicey_zpar_record_doubles(Rf.n_inst, NEL, T));  // (behind the parameter record: tran_pt_layout.h)
        for (int i = tid; i < SPICEY_TOP_FOLD_WORDS; i += T) c.tail[i] = fold[i];
      }
    }
    for (int i = tid; i < Qf.tail_n * 64; i += T) {  // tail records -> LDS (16 bytes each; no task = all zero)
      const int p = Qf.tail_first + (i >> 6), lane = i & 63;
      const bool have = (uint32_t)lane < Pf.ph_cnt[p];
      const uint32_t *src = Pf.rec16 + ((size_t)Pf.ph_first[p] + (have ? lane : 0)) * 4;
      for (int w = 0; w < 4; w++) c.tail[(size_t)i * 4 + w] = have ? src[w] : 0u;
    }
  });
  ex.phase(SPICEY_PH_PRO, [&](int tid) { const SpiceyProg Pf = ex.fresh(P); const SpiceyRun Rf = ex.fresh(R); TranPhases<K> ph{Pf, Rf, c, T}; ph.p1_static(tid); });
  ex.phase(SPICEY_PH_PRO, [&](int tid) { const SpiceyProg Pf = ex.fresh(P); const SpiceyRun Rf = ex.fresh(R); Ph2 p2{Pf, Rf, c, T, brem, zrem}; p2.a0_initial(tid, ex.template regs<Regs>(tid)); if (EP) p2.zpar_fill(tid); });
  if constexpr (SF) {  // step 0's stamps, by the phase B of every other form; then the fused form's slots into the same registers
    ex.phase(SPICEY_PH_PRO, [&](int tid) {
      const SpiceyProg Pf = ex.fresh(P); const SpiceyRun Rf = ex.fresh(R);
      Ph2 p2{Pf, Rf, c, T, brem, zrem};
      p2.b_stamp(tid, ex.template regs<Regs>(tid));
      SPICEY_SCHED_FENCE;
      const uint32_t *fuse = (const uint32_t *)(Rf.zpar + spicey_zpar_record_doubles(Rf.n_inst, NEL, T)) + SPICEY_TOP_FOLD_WORDS;
      p2.sf_load(tid, ex.template regs<Regs>(tid), fuse);
    });
  }
  unsigned long long solves = 0;
  int32_t code = 0;
  int64_t err_step = 0;
  int32_t err_iter = 0;
  if (c.flags[1]) { code = 1; }
  // loop control: a handful of scalars
  const int nL = P.nLevels;
  const int nS = P.nS;
  const int64_t steps = R.steps;
  const int dbg_empty = R.debug_empty_phases;
  // which phases have work: kept in a scalar mask so that the phase loop issues no loads
  unsigned long long active = 0, smask = 0;
  for (int p = 0; p < 2 * nL && p < 64; p++) {
    if (SPICEY_UNIFORM((int)P.ph_cnt[p]) != 0) active |= 1ull << p;
    if (SPICEY_UNIFORM((int)Q.st_cnt[p]) != 0) smask |= 1ull << p;
  }
  const int tail_n = Q.tail_n, tail_first = Q.tail_first;
  // (the tridiagonal top's two loop-control values ride in ONE scalar across the time loop and are unpacked inside it: every
  // further live scalar there costs a lane of a spill VGPR, and the 128-register build has none to give)
  int top_pack;
  {
    const int n0 = K == 1 ? P.pcr_n : 0;
    int S0 = 0;
    while ((1 << S0) < n0) S0++;
    top_pack = n0 | (S0 << 8);
  }
  const int pcr_n = top_pack & 0xff;
  // with a tridiagonal top the factor phases end at its level and the backward phases resume below it
  const int u_end = pcr_n > 0 ? P.pcr_level : (tail_n > 0 ? tail_first : nL);
  const int k_begin = pcr_n > 0 ? 2 * nL - P.pcr_level : (tail_n > 0 ? tail_first + tail_n : nL);
  // bit 16 = z_pre: Z's parameter fetch rides on the last backward phase (EP: on the last factor phase, and the source value
  // is parked by the last backward one — both must exist)
  top_pack |= (K == 1 && k_begin < 2 * nL && (!EP || u_end > 0)) ? 1 << 16 : 0;
  // No diodes and no switches: the matrix of every step is the matrix of step 0 (dt is fixed within a run), so its
  // factors stay in W and later steps run the right-hand-side column only.  Same operands, same order: the results
  // are bit-identical to refactoring (SURVEY.md §8(d) "solve-only" rate; the reference itself never reuses).
  top_pack |= (P.nD == 0 && nS == 0 && P.nDynEnt == 0 && !R.no_reuse) ? 1 << 17 : 0;  // bit 17 = linear
  top_pack |= (Ph2::DIAG && R.skip_risk != nullptr) ? 1 << 18 : 0;  // bit 18 = diagnostics: look at the stamped matrix after B (spicey_skip_risk)
  top_pack |= (K == 1 && pcr_n > 0 && Q.k_merge == k_begin && k_begin < 2 * nL - 1) ? 1 << 19 : 0;  // bit 19 = the first backward phase runs in the top's wave
  top_pack |= (PT < 0 && pt_run) ? 1 << 20 : 0;  // bit 20 = the phases take their arguments from the phase table (where that is a run-time choice)
  top_pack = SPICEY_UNIFORM(top_pack);
  if constexpr (FS) {
    static_assert(PT != 0 && EP && RA && OA && TR && UR && TF, "the fixed schedule: the table is on, every form below the fuse is taken");
    constexpr int PR_WIDE = 1, PR_NARROW = 2;  // (the issue priorities of GpuExecV2::phase: the two wide factor levels, every narrow one)
    constexpr bool IDLE = SpiceyHasIdleWaves<Exec>::value;
    for (int64_t step = 0; step <= steps && code == 0; step++) {
      int tp = top_pack;
      SPICEY_OPAQUE_S(tp);
      const int pcr_n = tp & 0xff, pcr_S = (tp >> 8) & 0xff;
      const uint32_t *ptw = c.tail + spicey_pt_base_words(pcr_n);
      // 1. U_0 from the resident record, 2. the resident factor levels below the folded one
      spicey_phase_at<PR_WIDE>(ex, SPICEY_PH_U0, [&](int tid) { spicey_u0_resident_phase<K, RMAX, NSV, NEL, OA>(c, ex.template regs<Regs>(tid)); });
      if (u_end > 2) spicey_phase_at<PR_WIDE>(ex, SPICEY_PH_U0 + 1, [&](int tid) { spicey_uk_phase_fs<K, RMAX, NSV, NEL, false, OA>(c, ex.template regs<Regs>(tid), 1); });
      for (int p = 2; p < u_end - 1; p++)
        spicey_phase_at<PR_NARROW>(ex, SPICEY_PH_U0 + (p < 30 ? p : 30), [&](int tid) { spicey_uk_phase_fs<K, RMAX, NSV, NEL, false, OA>(c, ex.template regs<Regs>(tid), p); });
      // 3. the folded top, the first backward phase behind it in the same wave, and Z's early fetch beside them
      auto early_fetch = [&](int tid) {
        SpiceyProg Pt{};
        SpiceyRun Rt{};
        spicey_pt_args_early(SpiceyPtLanes::run_block(ptw, tid), Pt, Rt);
        Rt.steps = steps;
        Ph2 p2{Pt, Rt, c, T, 0u, 0u, &P, &R, ptw};
        p2.z_early(tid, step, ex.template regs<Regs>(tid));
      };
      auto merged_k = [&](int lane) { spicey_uk_phase_fs<K, RMAX, NSV, NEL, true, OA>(c, ex.template regs<Regs>(lane), k_begin); };
      if constexpr (!IDLE) ex.phase(SPICEY_PH_U0 + (u_end - 1 < 30 ? u_end - 1 : 30), early_fetch);  // (an executor without idle waves: a phase of its own, where the folded level's was)
#if defined(__HIP_DEVICE_COMPILE__)
      auto top_all = [&](int lane, int, double *) {
        spicey_pcr_all_regs<K, true>(c, (const uint16_t *)(c.tail + 1024), pcr_n, pcr_S, lane);  // (all 64 lanes: nlanes = 64 below)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        merged_k(lane);
      };
      if constexpr (IDLE) ex.wave_lockstep_keep_then(64, 1, top_all, early_fetch);
      else ex.wave_lockstep_keep(64, 1, top_all);
#else
      auto top_staged = [&](int lane, int st, double *) {  // (the whole wave in one call, whichever lane the executor runs first)
        if (st == 0 && lane == 0) spicey_top_fold_wave<K>(c, c.tail, (const uint16_t *)(c.tail + 1024), pcr_n, pcr_S);
        if (st > pcr_S) merged_k(lane);
      };
      if constexpr (IDLE) ex.wave_lockstep_keep_then(64, pcr_S + 2, top_staged, early_fetch);
      else ex.wave_lockstep_keep(64, pcr_S + 2, top_staged);
#endif
      // 4. the remaining backward phases; the last parks the source value that the early fetch left in a register
      for (int p = k_begin + 1; p < 2 * nL - 1; p++) {
        const int l = 2 * nL - 1 - p;
        spicey_phase_at<PR_NARROW>(ex, SPICEY_PH_K0 + (l < 31 ? l : 31), [&](int tid) { spicey_uk_phase_fs<K, RMAX, NSV, NEL, true, OA>(c, ex.template regs<Regs>(tid), p); });
      }
      spicey_phase_at<PR_NARROW>(ex, SPICEY_PH_K0, [&](int tid) {
        spicey_uk_phase_fs<K, RMAX, NSV, NEL, true, OA>(c, ex.template regs<Regs>(tid), 2 * nL - 1);  // (level 0: the leaves)
        SPICEY_SCHED_FENCE;  // after the tasks, not among them: their registers are free by now
        SpiceyProg Pt{};
        SpiceyRun Rt{};
        spicey_pt_args(ptw, tid, Pt, Rt);
        Ph2 p2{Pt, Rt, c, T, 0u, 0u, &P, &R};
        p2.z_src_park(tid, ex.template regs<Regs>(tid).srcn);
      });
      if (c.flags[1]) { code = 1; err_step = step; err_iter = 0; break; }
      solves += (unsigned long long)c.valid[0];
      // 5. Z with the stamp arithmetic, 6. its second phase
      spicey_phase_at<0>(ex, SPICEY_PH_Z, [&](int tid) {
        const uint32_t *ptz = c.tail + spicey_pt_base_words(top_pack & 0xff);
        SpiceyProg Pt{};
        SpiceyRun Rt{};
        spicey_pt_args_z(SpiceyPtLanes::run_block(ptz, tid), Pt, Rt);
        Rt.steps = steps;
        Ph2 p2{Pt, Rt, c, T, 0u, 0u, &P, &R, ptz};
        p2.z_record(tid, step, ex.template regs<Regs>(tid), true);  // (the iteration count: behind the loop)
      });
      spicey_phase_at<0>(ex, SPICEY_PH_Z2, [&](int tid) {
        Ph2 p2{P, R, c, T, 0u, 0u};
        p2.z_fuse(tid, step == steps, ex.template regs<Regs>(tid));
      });
    }
    // the iteration counts of the recorded steps — 1 each: such a run never re-iterates — with all threads, and nothing at or
    // behind a failing step
    ex.phase(SPICEY_PH_PRO, [&](int tid) {
      const SpiceyRun Rf = ex.fresh(R);
      if (Rf.iters && c.valid[0]) {
        int32_t *it = Rf.iters + (size_t)c.inst[0] * (size_t)(steps + 1);
        const int64_t done = code ? err_step : steps + 1;
        for (int64_t i = tid; i < done; i += T) it[i] = 1;
      }
    });
  } else
  // (The loop above is this loop written out for one plan: phase order, tags, priorities, the merged phase's id, the error
  // break ahead of Z, the solve count and what `iters` holds after an error are copied by hand.  Whoever changes one of
  // them here changes it there; tests/test_fixed_schedule.py and test_fixed_schedule_gpu.py hold the two against each other.)
  for (int64_t step = 0; step <= steps && code == 0; step++) {
    int iter = 0;
    for (;;) {
      int tp = top_pack;
      SPICEY_OPAQUE_S(tp);
      const int pcr_n = tp & 0xff, pcr_S = (tp >> 8) & 0xff;
      const bool linear = (tp >> 17) & 1;
      // (with a table u_end = pcr_level rows of factor phases come first, the backward phases from k_begin on follow)
      const bool pt_on = PT >= 0 ? PT == 1 : ((tp >> 20) & 1) != 0;
      const uint32_t *ptw = c.tail + spicey_pt_base_words(pcr_n);
      const bool pt_bz = !HYB && pt_on;  // (hybrid builds: B and Z read many more fields; they keep the scalar loads)
      if constexpr (!SF)  // (SF: the previous step's Z, or the prologue, has stamped)
      ex.phase(SPICEY_PH_B, [&](int tid) {
        if (pt_bz) {
          SpiceyProg Pt{};
          SpiceyRun Rt{};
          spicey_pt_args(ptw, tid, Pt, Rt);
          // (fresh build: nKeep rides in the spare word of phase 0's row — spicey_build_resident — so that the run-wide block,
          // and with it every other build, is what it was)
          if (Ph2::FRESH) Pt.nKeep = (int32_t)SpiceyPtLanes::row(ptw, tid, 0).u32(7);
          Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R, ptw, nullptr};
          p2.template b_phase<UR>(tid, step, ex.template regs<Regs>(tid), linear && step > 0);
        } else {
          const SpiceyProg Pf = ex.fresh(P);
          const SpiceyRun Rf = ex.fresh(R);
          Ph2 p2{Pf, Rf, c, T, brem, zrem, nullptr, nullptr, nullptr, &Q};
          p2.template b_phase<UR>(tid, step, ex.template regs<Regs>(tid), linear && step > 0);
        }
      });
      if (Ph2::DIAG && ((tp >> 18) & 1) && !(linear && step > 0))
        ex.phase(SPICEY_PH_S, [&](int tid) {
          const SpiceyProg Pf = ex.fresh(P);
          const SpiceyRun Rf = ex.fresh(R);
          spicey_skip_risk<K, HYB>(Pf, Rf, c, tid, T, linear ? (unsigned long long)(steps + 1) : 1ull);
        });
      for (int d = 0; d < dbg_empty; d++) ex.phase(SPICEY_PH_S, [&](int) {});  // diagnostics: cost of a bare phase
      // factor levels [0, u_end) | tail [u_end, k_begin) by one wave | backward levels [k_begin, 2 nL)
      constexpr bool IDLE = EP && SpiceyHasIdleWaves<Exec>::value;
      const bool z_early = EP && ((tp >> 16) & 1) != 0;
      const int kmerge = (tp >> 19) & 1;
      // EP: Z's parameter record and the next source value of thread tid (whole waves arrive here)
      auto early_fetch = [&](int tid) {
        if (!z_early) {
          Ph2 p2{P, R, c, T, brem, zrem};
          p2.z_early_none(ex.template regs<Regs>(tid));
        } else if (RA && pt_bz) {
          SpiceyProg Pt{};
          SpiceyRun Rt{};
          spicey_pt_args_early(SpiceyPtLanes::run_block(ptw, tid), Pt, Rt);
          Rt.steps = steps;
          Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R, ptw};
          p2.z_early(tid, step, ex.template regs<Regs>(tid));
        } else if (pt_bz) {
          SpiceyProg Pt{};
          SpiceyRun Rt{};
          spicey_pt_args(ptw, tid, Pt, Rt);
          Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R};
          p2.z_early(tid, step, ex.template regs<Regs>(tid));
        } else {
          const SpiceyProg Pf = ex.fresh(P);
          const SpiceyRun Rf = ex.fresh(R);
          Ph2 p2{Pf, Rf, c, T, brem, zrem};
          p2.z_early(tid, step, ex.template regs<Regs>(tid));
        }
      };
      for (int p = 0, u_gen = (z_early && !IDLE) ? u_end - 1 : u_end; p < u_gen; p++) {
        if (p < 64 ? !((active >> p) & 1) : P.ph_cnt[p] == 0) continue;
        if constexpr (TF) {
          if (p == u_end - 1) continue;  // (the top's head runs this level)
        }
        if (HYB && p == 0) {
          // hybrid workspace: phase 0 eliminates the leaves, whose own entries are read from the global array (one L2 round
          // trip for the whole level; every target is in LDS)
          ex.phase(SPICEY_PH_U0, [&](int tid) {
            spicey_uk_phase<K, RMAX, NSV, NEL, false, HYB>(P, Q, SpiceyPt{ptw, pt_on, 0}, c, ex.template regs<Regs>(tid), tid, T, 0, ((smask >> 0) & 1) != 0, linear && step > 0);
          });
          continue;
        }
        if constexpr (UR) {
          if (p == 0) {  // (the record is in registers: load_resident)
            ex.phase(SPICEY_PH_U0, [&](int tid) { spicey_u0_resident_phase<K, RMAX, NSV, NEL, OA>(c, ex.template regs<Regs>(tid)); });
            continue;
          }
        }
        ex.phase(SPICEY_PH_U0 + (p < 30 ? p : 30), [&](int tid) {
          spicey_uk_phase<K, RMAX, NSV, NEL, false, false, OA, UR>(P, Q, SpiceyPt{ptw, pt_on, p}, c, ex.template regs<Regs>(tid), tid, T, p, p < 64 ? ((smask >> p) & 1) != 0 : true, linear && step > 0);
        });
      }
      // EP without idle waves: the last factor phase is peeled and fetches at its tail, after its tasks (it runs for its
      // tail even where it has no task)
      if (EP && !IDLE && z_early) {
        const int p = u_end - 1;
        const bool act = !TF && (p < 64 ? ((active >> p) & 1) != 0 : P.ph_cnt[p] != 0);  // (TF: the top's head runs this level)
        ex.phase(SPICEY_PH_U0 + (p < 30 ? p : 30), [&](int tid) {
          bool u0_done = false;
          if constexpr (UR) {
            if (act && p == 0) { spicey_u0_resident_phase<K, RMAX, NSV, NEL, OA>(c, ex.template regs<Regs>(tid)); u0_done = true; }
          }
          if (act && !u0_done) spicey_uk_phase<K, RMAX, NSV, NEL, false, false, OA, UR>(P, Q, SpiceyPt{ptw, pt_on, p}, c, ex.template regs<Regs>(tid), tid, T, p, p < 64 ? ((smask >> p) & 1) != 0 : true, linear && step > 0);
          SPICEY_SCHED_FENCE;
          early_fetch(tid);
        });
      } else if (EP && !IDLE) {
        early_fetch(0);
      }
      if (pcr_n > 0) {
        // (kmerge: wave 0 goes on with the first backward phase below the top — its records are resident in this wave's
        // slots, its rows need unknowns of the top only, and the LDS operations of one wave execute in order)
        auto merged_k = [&](int lane) {
          spicey_uk_phase<K, RMAX, NSV, NEL, true, false, OA>(P, Q, SpiceyPt{ptw, pt_on, u_end}, c, ex.template regs<Regs>(lane), lane, T, k_begin, false);
        };
#if defined(__HIP_DEVICE_COMPILE__)
        if (TF || (pcr_S >= 1 && pcr_S <= 6)) {  // (TF: a register-exchange-top run, 1 .. 6 stages by its plan)
          auto top_all = [&](int lane, int, double *) {
            if constexpr (TR) spicey_pcr_all_regs<K, TF>(c, (const uint16_t *)(c.tail + 1024), pcr_n, pcr_S, lane);  // (all 64 lanes: nlanes = 64 below)
            else spicey_pcr_all<K>(c, (double *)c.tail, (const uint16_t *)(c.tail + 1024), pcr_n, pcr_S, lane);
            if (kmerge) {
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
              __builtin_amdgcn_wave_barrier();
              merged_k(lane);
            }
          };
          if constexpr (IDLE) ex.wave_lockstep_keep_then(64, 1, top_all, early_fetch);
          else ex.wave_lockstep_keep(64, 1, top_all);
        } else
#endif
        {
          auto top_staged = [&](int lane, int st, double *own) {
            if constexpr (TF) {  // (host executors only — the whole wave in one call, whichever lane the executor runs first)
#if !defined(__HIP_DEVICE_COMPILE__)
              if (st == 0 && lane == 0) spicey_top_fold_wave<K>(c, c.tail, (const uint16_t *)(c.tail + 1024), pcr_n, pcr_S);
#endif
              if (st > pcr_S) merged_k(lane);
              return;
            }
            if (st <= pcr_S) spicey_pcr_stage<K>(c, (double *)c.tail, (const uint16_t *)(c.tail + 1024), pcr_n, pcr_S, lane, st, own);
            else merged_k(lane);
          };
          if constexpr (IDLE) ex.wave_lockstep_keep_then(64, pcr_S + 1 + kmerge, top_staged, early_fetch);
          else ex.wave_lockstep_keep(64, pcr_S + 1 + kmerge, top_staged);
        }
      } else {
        if (k_begin > u_end)
        // the record of level l + 1 is fetched (LDS) while level l executes: one round trip less on the serial chain
        ex.tail_phase(SPICEY_PH_U0 + 31, k_begin - u_end,
                      [&](int tid, int lvl, uint32_t *r) {
                        const uint32_t *q = c.tail + ((size_t)lvl * 64 + tid) * 4;
                        r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; r[3] = q[3];
                      },
                      [&](int, int lvl, const uint32_t *r) {
                        auto ovf = [&]() -> const uint16_t * { return spicey_fresh(P).ovf16; };
                        if (u_end + lvl < nL) spicey_exec_rec16<K, false, false, SpiceyShapeKind<RMAX, NSV, NEL>::fresh>(c, ovf, r[0], r[1], r[2], r[3], (linear && step > 0) ? (uint32_t)spicey_fresh(P).xoff : 0u);
                        else spicey_exec_rec16<K, true>(c, ovf, r[0], r[1], r[2], r[3]);
                      });
        // (no top to ride on: a phase of its own — in this very branch, so that every path through the iteration visibly
        // defines the registers)
        if (IDLE) ex.phase(SPICEY_PH_S, early_fetch);
      }
      for (int p = k_begin + kmerge; p < 2 * nL - 1; p++) {
        const int l = 2 * nL - 1 - p;
        ex.phase(SPICEY_PH_K0 + (l < 31 ? l : 31), [&](int tid) {
          spicey_uk_phase<K, RMAX, NSV, NEL, true, false, OA>(P, Q, SpiceyPt{ptw, pt_on, p - k_begin + u_end}, c, ex.template regs<Regs>(tid), tid, T, p, p < 64 ? ((smask >> p) & 1) != 0 : true);
        });
      }
      // the last backward phase (level 0) is peeled: it also issues Z's parameter fetch.  (Every path through the
      // iteration defines the prefetch registers, so they are not live around the time loop.)
      if (k_begin < 2 * nL) {
        const int p = 2 * nL - 1;
        ex.phase(SPICEY_PH_K0, [&](int tid) {
          spicey_uk_phase<K, RMAX, NSV, NEL, true, HYB, OA>(P, Q, SpiceyPt{ptw, pt_on, p - k_begin + u_end}, c, ex.template regs<Regs>(tid), tid, T, p, p < 64 ? ((smask >> p) & 1) != 0 : true);  // (level 0: the leaves)
          SPICEY_SCHED_FENCE;  // after the tasks, not among them: their registers are free by now
          if (K == 1 && EP) {  // (the source value that early_fetch left in a register: Z reads the slot, nothing before it does)
            if (!z_early) return;
            if (pt_bz) {
              SpiceyProg Pt{};
              SpiceyRun Rt{};
              spicey_pt_args(ptw, tid, Pt, Rt);
              Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R};
              p2.z_src_park(tid, ex.template regs<Regs>(tid).srcn);
            } else {
              const SpiceyProg Pf = ex.fresh(P);
              const SpiceyRun Rf = ex.fresh(R);
              Ph2 p2{Pf, Rf, c, T, brem, zrem};
              p2.z_src_park(tid, ex.template regs<Regs>(tid).srcn);
            }
          } else if (K == 1) {
            if (pt_bz) {
              SpiceyProg Pt{};
              SpiceyRun Rt{};
              spicey_pt_args(ptw, tid, Pt, Rt);
              Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R};
              p2.z_prefetch(tid, step, 0, ex.template regs<Regs>(tid));
            } else {
              const SpiceyProg Pf = ex.fresh(P);
              const SpiceyRun Rf = ex.fresh(R);
              Ph2 p2{Pf, Rf, c, T, brem, zrem};
              p2.z_prefetch(tid, step, 0, ex.template regs<Regs>(tid));
            }
          }
        });
      } else if (K == 1 && !EP) {
        Ph2 p2{P, R, c, T, brem, zrem};
        p2.z_prefetch_none(ex.template regs<Regs>(0));
      }
      if (c.flags[1]) { code = 1; err_step = step; err_iter = iter; break; }
      if (nS == 0) break;
      ex.phase(SPICEY_PH_S, [&](int tid) { const SpiceyProg Pf = ex.fresh(P); const SpiceyRun Rf = ex.fresh(R); TranPhases<K> ph{Pf, Rf, c, T}; ph.s_switches(tid); });
      const int switched = c.flags[0];
      if (!switched || iter == SPICEY_MAX_ITER - 1) break;
      iter++;
      ex.phase(SPICEY_PH_A, [&](int tid) { const SpiceyProg Pf = ex.fresh(P); const SpiceyRun Rf = ex.fresh(R); Ph2 p2{Pf, Rf, c, T, brem, zrem}; p2.a_reiterate(tid); });
    }
    if (code) break;
    {
      int nvalid = 0;
      for (int k = 0; k < K; k++) nvalid += c.valid[k];
      solves += (unsigned long long)(iter + 1) * (unsigned long long)nvalid;
    }
    ex.phase(SPICEY_PH_Z, [&](int tid) {
      if (RA && !HYB && (PT >= 0 ? PT == 1 : ((top_pack >> 20) & 1) != 0)) {
        const uint32_t *ptz = c.tail + spicey_pt_base_words(top_pack & 0xff);
        SpiceyProg Pt{};
        SpiceyRun Rt{};
        spicey_pt_args_z(SpiceyPtLanes::run_block(ptz, tid), Pt, Rt);
        Rt.steps = steps;
        Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R, ptz};
        const uint32_t st32 = (uint32_t)SPICEY_UNIFORM((int)(uint32_t)step);
        if (tid == 0 && Rt.iters && c.valid[0]) Rt.iters[st32] = iter + 1;  // (this instance's row: spicey_pt_rebase_ready)
        p2.z_record(tid, step, ex.template regs<Regs>(tid), ((top_pack >> 16) & 1) != 0);
      } else if (!HYB && (PT >= 0 ? PT == 1 : ((top_pack >> 20) & 1) != 0)) {
        SpiceyProg Pt{};
        SpiceyRun Rt{};
        spicey_pt_args(c.tail + spicey_pt_base_words(top_pack & 0xff), tid, Pt, Rt);
        Ph2 p2{Pt, Rt, c, T, brem, zrem, &P, &R};
        if (tid == 0 && Rt.iters)
          for (int k = 0; k < K; k++)
            if (c.valid[k]) Rt.iters[(size_t)c.inst[k] * (size_t)(steps + 1) + (size_t)step] = iter + 1;
        p2.z_record(tid, step, ex.template regs<Regs>(tid), ((top_pack >> 16) & 1) != 0);
      } else {
        const SpiceyRun Rf = ex.fresh(R);
        const SpiceyProg Pf = ex.fresh(P);
        Ph2 p2{Pf, Rf, c, T, brem, zrem};
        if (tid == 0 && Rf.iters)
          for (int k = 0; k < K; k++)
            if (c.valid[k]) Rf.iters[(size_t)c.inst[k] * (size_t)(steps + 1) + (size_t)step] = iter + 1;
        p2.z_record(tid, step, ex.template regs<Regs>(tid), ((top_pack >> 16) & 1) != 0);
      }
    });
    if constexpr (SF) {
      ex.phase(SPICEY_PH_Z2, [&](int tid) {  // (the rows, from registers: no argument of the run is read)
        Ph2 p2{P, R, c, T, brem, zrem};
        p2.z_fuse(tid, step == steps, ex.template regs<Regs>(tid));
      });
    }
  }
  ex.phase(SPICEY_PH_PRO, [&](int tid) {
    if (tid == 0) {
      const SpiceyRun Rf = ex.fresh(R);
      Rf.status[wg * 4 + 0] = code;
      Rf.status[wg * 4 + 1] = c.flags[2];
      Rf.status[wg * 4 + 2] = (int32_t)err_step;
      Rf.status[wg * 4 + 3] = err_iter;
      Rf.solves[wg] = solves;
    }
  });
}
