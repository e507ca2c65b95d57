// tran_sens_exec.h — sensitivities and corners of transient measurements: the one definition of the deterministic design written
// into a transient run's value arrays and of the reduction of the scalars x [n_inst][n_scalar] across the design's instances,
// used by the kernels of tran_sens.hip and by the CPU harness of tests/tran_sens_host (compiled without FMA contraction on both
// sides, so the two give the same bits).  The scalars themselves are tran_mc_exec.h's (spicey_tmc_scalar), unchanged.
//
// The design.  One thread per (instance s, element e), e over the nE = nR + nC + nL elements in the order R, C, L, writes
// v' = v g — one product; a resistor stays in ohms, the transient kernels form 1.0 / R themselves — with
//   ONE_AT_A_TIME   act [nA] strictly ascending element indices, step [nA]: instance 0 is nominal; instance 1 + 2a has element
//                   act[a] at g = 1.0 + step[a], instance 2 + 2a has it at g = 1.0 - step[a]; every other g is 1.0.
//   LEVELS          lvl [n_inst][nE] int8 in {-1, 0, +1}, tol [nE]: g = 1.0 + (double)lvl tol[e] (a product, then a sum).
//
// The reduction.  One wave per scalar j; lane l handles the active elements a = l, l + 64, ...  With x0 = x[0][j],
// xp = x[1 + 2a][j], xm = x[2 + 2a][j], h = step[a], t = tol_act[a] (the tolerance of element act[a]):
//   d = (xp - xm) / (2.0 h)                the change of the scalar per unit relative change of the element
//   c = ((xp - x0) + (xm - x0)) / (h h)    the curvature
//   sign = +1 if d > 0, -1 if d < 0, else 0 (int8)
// An element is a number iff instances 0, 1 + 2a and 2 + 2a are valid, none of x0, xp, xm is NaN, and neither d nor c comes
// out NaN (inf - inf); otherwise d = c = the NaN 0x7ff8000000000000 and sign = 0.  Over the numbers, in ascending a per lane:
//   wc += |d| t, rss2 += (d t) (d t) — each lane from +0.0 —, n_num, n_interior = #{|d| < |c| t}, and the lowest a with the
//   largest m = |d| t (a later a replaces an earlier one only if its m is greater).
// The lanes meet by s[l] += s[l + stride], stride 32 .. 1 (counts by +; of two largest m the greater, of equal ones the lower a).
//   d_sens  [n_scalar][nA][2] = {d, c}      d_sign [n_scalar][nA] int8
//   d_bound [n_scalar][8]     = {x0, wc, rss2, n_num, a_max, contrib_max, n_interior, 0}
// With n_num = 0: wc = rss2 = +0.0, a_max = -1, contrib_max = +0.0.  Counts and indices are stored as doubles.  No square root
// runs here; nothing depends on the thread count.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tran_mc_exec.h"

#define SPICEY_TS_BOUND_ROW 8  // doubles of a d_bound row

// A validated design with the buffers it runs on (tran_sens.h: spicey_ts_design_judge).  act, step, lvl and tol lie in the workspace.
struct SpiceyTsDesignArgs {
  const double *R, *C, *L;  // [n_inst][n<kind>] nominal values
  double *oR, *oC, *oL;     // [n_inst][n<kind>] what the run reads
  const int32_t *act;       // [nA]            ONE_AT_A_TIME
  const double *step;       // [nA]
  const int8_t *lvl;        // [n_inst][nE]    LEVELS
  const double *tol;        // [nE]
  int32_t n_inst, nR, nC, nL, nA, mode;
};

// The factor of element e in instance s.
SPICEY_MEAS_HD double spicey_ts_gain(const SpiceyTsDesignArgs &A, int64_t s, int32_t e) {
  if (A.mode == SPICEY_TS_LEVELS) {
    const int64_t nE = (int64_t)A.nR + A.nC + A.nL;
    return 1.0 + (double)A.lvl[s * nE + e] * A.tol[e];
  }
  if (s == 0) return 1.0;
  const int64_t a = (s - 1) >> 1;
  if (A.act[a] != e) return 1.0;
  return ((s - 1) & 1) ? 1.0 - A.step[a] : 1.0 + A.step[a];
}

// Thread idx = s * nE + e of the design kernel.
SPICEY_MEAS_HD void spicey_ts_design(const SpiceyTsDesignArgs &A, int64_t idx) {
  const int64_t nE = (int64_t)A.nR + A.nC + A.nL;
  const int64_t s = idx / nE;
  const int32_t e = (int32_t)(idx - s * nE);
  const double g = spicey_ts_gain(A, s, e);
  if (e < A.nR) {
    const int64_t at = s * A.nR + e;
    A.oR[at] = A.R[at] * g;
  } else if (e < A.nR + A.nC) {
    const int64_t at = s * A.nC + (e - A.nR);
    A.oC[at] = A.C[at] * g;
  } else {
    const int64_t at = s * A.nL + (e - A.nR - A.nC);
    A.oL[at] = A.L[at] * g;
  }
}

// A validated reduction (tran_sens.h: spicey_ts_reduce_judge).  valid, step and tol_act lie in the workspace; valid is null when
// every instance is valid.  n_inst = 1 + 2 nA.
struct SpiceyTsReduceArgs {
  const double *x;        // [n_inst][n_scalar], what the scalar kernel wrote
  const uint8_t *valid;   // [n_inst]
  const double *step;     // [nA]
  const double *tol_act;  // [nA]
  double *sens;           // [n_scalar][nA][2]
  int8_t *sign;           // [n_scalar][nA]
  double *bound;          // [n_scalar][8]
  int32_t n_inst, n_scalar, nA, pad;
};

SPICEY_MEAS_HD bool spicey_ts_ok(const SpiceyTsReduceArgs &A, int64_t s) { return !A.valid || A.valid[s]; }

// What lane `lane` brings: its sums and counts, and its lowest element with the largest |d| t (a = -1: none).
struct SpiceyTsPartial { double wc, rss2, m; int32_t n_num, n_int, a; };

// Lane `lane` of scalar j: writes d_sens and d_sign of its elements and forms its partial.
SPICEY_MEAS_HD void spicey_ts_lane(const SpiceyTsReduceArgs &A, int32_t j, int32_t lane, SpiceyTsPartial *p) {
  p->wc = 0.0; p->rss2 = 0.0; p->m = -1.0; p->n_num = 0; p->n_int = 0; p->a = -1;
  const double nan = spicey_mc_double(SPICEY_TMC_NAN_BITS);
  const double x0 = A.x[j];
  const bool ok0 = spicey_ts_ok(A, 0) && x0 == x0;
  for (int32_t a = lane; a < A.nA; a += SPICEY_MC_LANES) {
    const int64_t sp = 1 + 2 * (int64_t)a, sm = sp + 1;
    const double xp = A.x[sp * A.n_scalar + j], xm = A.x[sm * A.n_scalar + j];
    const double h = A.step[a], t = A.tol_act[a];
    double d = (xp - xm) / (2.0 * h);
    double c = ((xp - x0) + (xm - x0)) / (h * h);
    const bool num = ok0 && spicey_ts_ok(A, sp) && spicey_ts_ok(A, sm) && xp == xp && xm == xm && d == d && c == c;
    int8_t sign = 0;
    if (num) {
      sign = d > 0.0 ? 1 : d < 0.0 ? -1 : 0;
      const double m = fabs(d) * t, dt = d * t;
      p->wc = p->wc + m;
      p->rss2 = p->rss2 + dt * dt;
      p->n_num++;
      if (fabs(d) < fabs(c) * t) p->n_int++;
      if (m > p->m) { p->m = m; p->a = a; }
    } else {
      d = nan;
      c = nan;
    }
    const int64_t at = (int64_t)j * A.nA + a;
    A.sens[2 * at] = d;
    A.sens[2 * at + 1] = c;
    A.sign[at] = sign;
  }
}

// How lane l takes lane l + stride's partial.
SPICEY_MEAS_HD void spicey_ts_meet(SpiceyTsPartial *p, const SpiceyTsPartial &q) {
  p->wc = p->wc + q.wc;
  p->rss2 = p->rss2 + q.rss2;
  p->n_num += q.n_num;
  p->n_int += q.n_int;
  if (q.a >= 0 && (p->a < 0 || q.m > p->m || (q.m == p->m && q.a < p->a))) { p->m = q.m; p->a = q.a; }
}

// What lane 0 writes once the partials have met.
SPICEY_MEAS_HD void spicey_ts_bound_row(const SpiceyTsReduceArgs &A, int32_t j, const SpiceyTsPartial &p) {
  double *dst = A.bound + (int64_t)j * SPICEY_TS_BOUND_ROW;
  const double x0 = A.x[j];
  dst[0] = (spicey_ts_ok(A, 0) && x0 == x0) ? x0 : spicey_mc_double(SPICEY_TMC_NAN_BITS);
  dst[1] = p.wc; dst[2] = p.rss2; dst[3] = (double)p.n_num; dst[4] = (double)p.a;
  dst[5] = p.a >= 0 ? p.m : 0.0;
  dst[6] = (double)p.n_int; dst[7] = 0.0;
}
