// fit_exec.h — sizing elements to measured goals by damped least squares (Levenberg-Marquardt): the one definition of the design
// over the element GAINS of a transient run's instances and of the dense update behind one evaluation, used by the kernels of
// fit.hip and by the CPU harness of tests/fit_host (compiled without FMA contraction on both sides, so the two give the same bits).
//
// A handle of n_inst = n_ckt W instances, W = 1 + 2 nA; instance c W belongs to circuit c and is nominal, instance c W + 1 + 2a has
// active element a at +h_a, instance c W + 2 + 2a has it at -h_a.  act [nA] are strictly ascending indices into the R, C, L order
// (the design looks its element up in them).  The unknowns are gains g [n_ckt][nA] on the handle's own values; a
// resistor stays in ohms.  No exp, log or sqrt runs here.
//
// The design.  One thread per (instance s, element e):  an inactive element gets v' = v; the active element a of a perturbed
// instance gets v' = v gp with gp = g_a (1.0 + h_a) or g_a (1.0 - h_a); the nominal's, and every other instance's, gets v' = v g_a —
// every product rounded on its own.
//
// The update.  One workgroup of SPICEY_FIT_THREADS per circuit whose done[c] is 0, every phase followed by a barrier, on the
// circuit's rows of x [n_inst][n_scalar], the instances' validity and its goals [n_scalar] of {kind, lo, hi, weight}.  Every
// product, quotient, sum and difference is rounded on its own; every sum runs in ascending index from +0.0 in ONE thread.
//   residual   r_j = w_j (x0_j - lo_j) (EQ), else w_j times the amount by which the bound is exceeded (x0_j - hi_j > 0 above,
//              x0_j - lo_j < 0 below), else +0.0; goal j is active iff it is EQ or r_j != 0; F = sum_j r_j r_j.  An invalid nominal
//              or a NaN x0_j: the point is not evaluable, F = +inf.
//   accept     iff first (the record's flag: the circuit's first update) and F is finite, or not first and F < F_good.  Then
//              J[j][a] = w_j ((x+_j - x-_j) / (2.0 h_a)) over the active j; a column with an invalid instance or a NaN entry is
//              frozen (zeroed, counted in n_frozen); A = J^T J, b = -(J^T r), sums over the active j alone; A, b, g_good = g,
//              F_good = F and n_frozen go into the circuit's state in the workspace; lambda = lambda0 (first) or lambda lam_down.
//              An accepted F <= f_tol converges at once (status 0), nothing is solved.
//   reject     lambda = lambda lam_up; lambda > lam_max: status 5 (stalled).  A first point that is not evaluable: status 2.
//   solve      M = A, M[a][a] = A[a][a] + lambda A[a][a], a zero diagonal becomes 1.0, column nA = b; Gaussian elimination
//              with partial pivoting in the order of pss_exec.h (the LOWEST row of the largest magnitude, |pivot| < pivot_min:
//              status 3), column-oriented back substitution.
//   step       d_a = delta_a clamped to +-max_step (a delta that is not finite: status 4); max|d|; an accepted point with
//              max|d| <= x_tol converges (status 0); else g_a = g_good_a (1.0 + d_a) clamped to [g_lo_a, g_hi_a] (n_clamped), status 1.
// With every status but 1 g[c] = g_good[c]: the gains that come back belong to a point that was evaluated.  Status 0 sets
// done[c] = 1, a status >= 2 sets done[c] = status: the circuit is frozen.
//   rows [n_ckt][8] = {F, F_good, lambda, accepted, status, max|d|, n_frozen, n_clamped}
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/spicey_hip.h"
#include "pss_exec.h"  // the pivot search: SpiceyPssPiv, spicey_pss_piv_lane, spicey_pss_piv_meet

#define SPICEY_FIT_HD SPICEY_PSS_HD
#define SPICEY_FIT_MAX_NA 128    // active elements of one circuit (the matrix lives in LDS)
#define SPICEY_FIT_THREADS 256   // the update's workgroup; the design's too
#define SPICEY_FIT_LANES SPICEY_PSS_LANES

// A validated call with the buffers it runs on (fit.h: spicey_fit_judge).  act .. valid lie in the workspace's heads, state behind them.
struct SpiceyFitArgs {
  const double *R, *C, *L;  // [n_inst][n<kind>] the handle's own values            design
  double *oR, *oC, *oL;     // [n_inst][n<kind>] what the run reads
  double *g;                // [n_ckt][nA]
  const double *x;          // [n_inst][n_scalar]                                  update
  double *rows;             // [n_ckt][8]
  int32_t *done;            // [n_ckt]
  const int32_t *act;       // [nA]
  const double *step;       // [nA]
  const double *g_lo, *g_hi;  // [n_ckt][nA]
  const SpiceyFitGoal *goals;  // [n_ckt][n_scalar]
  const uint8_t *valid;     // [n_inst], or null: every instance is valid
  double *state;            // [n_ckt][spicey_fit_state_doubles(nA)]
  double lambda0, lam_up, lam_down, lam_max, max_step, x_tol, f_tol, pivot_min;
  int32_t n_ckt, nA, nR, nC, nL, n_scalar, first, pad;
};

// One circuit's state between updates: A [nA][nA] | b [nA] | g_good [nA] | F_good | lambda | n_frozen.
SPICEY_FIT_HD int64_t spicey_fit_state_doubles(int32_t nA) { return (int64_t)nA * nA + 2 * (int64_t)nA + 3; }
SPICEY_FIT_HD bool spicey_fit_finite(double v) { return v - v == 0.0; }

// Thread idx = s * nE + e of the design kernel.
SPICEY_FIT_HD void spicey_fit_design(const SpiceyFitArgs &A, int64_t idx) {
  const int64_t nE = (int64_t)A.nR + A.nC + A.nL;
  const int32_t W = 1 + 2 * A.nA;
  const int64_t s = idx / nE;
  const int32_t e = (int32_t)(idx - s * nE);
  const int64_t c = s / W;
  const int32_t j = (int32_t)(s - c * W);
  int32_t a = -1;
  for (int32_t k = 0; k < A.nA; k++)
    if (A.act[k] == e) a = k;
  double gain = 1.0;
  if (a >= 0) {
    gain = A.g[c * A.nA + a];
    if (j == 1 + 2 * a) gain = gain * (1.0 + A.step[a]);
    else if (j == 2 + 2 * a) gain = gain * (1.0 - A.step[a]);
  }
  const double *src;
  double *dst;
  int64_t at;
  if (e < A.nR) { at = s * A.nR + e; src = A.R; dst = A.oR; }
  else if (e < A.nR + A.nC) { at = s * A.nC + (e - A.nR); src = A.C; dst = A.oC; }
  else { at = s * A.nL + (e - A.nR - A.nC); src = A.L; dst = A.oL; }
  dst[at] = a >= 0 ? src[at] * gain : src[at];
}

// What the phases of one circuit's update share besides the matrix (static LDS on the device).
struct SpiceyFitShared {
  double delta[SPICEY_FIT_MAX_NA];
  int32_t frz[SPICEY_FIT_MAX_NA];
  double F, lam, maxd, minpiv;
  int32_t accepted, status, solve, piv, n_frozen, n_clamped, bad, pad;
};

// The residual of goal G at x0 (x0 is not NaN).
SPICEY_FIT_HD double spicey_fit_resid(const SpiceyFitGoal &G, double x0) {
  if (G.kind == SPICEY_FIT_EQ) return G.weight * (x0 - G.lo);
  if (G.kind != SPICEY_FIT_AT_LEAST && x0 > G.hi) return G.weight * (x0 - G.hi);
  if (G.kind != SPICEY_FIT_AT_MOST && x0 < G.lo) return G.weight * (x0 - G.lo);
  return 0.0;
}
SPICEY_FIT_HD bool spicey_fit_active(const SpiceyFitGoal &G, double r) { return G.kind == SPICEY_FIT_EQ || r != 0.0; }
SPICEY_FIT_HD bool spicey_fit_ok(const SpiceyFitArgs &A, int64_t s) { return !A.valid || A.valid[s]; }
// J[j][a] of circuit c (goal j is active).
SPICEY_FIT_HD double spicey_fit_jac(const SpiceyFitArgs &A, int32_t c, const SpiceyFitGoal &G, int32_t j, int32_t a) {
  const int64_t sp = (int64_t)c * (1 + 2 * A.nA) + 1 + 2 * a;
  const double xp = A.x[sp * A.n_scalar + j], xm = A.x[(sp + 1) * A.n_scalar + j];
  return G.weight * ((xp - xm) / (2.0 * A.step[a]));
}

// Thread 0: F at the nominal, accept or reject, lambda, and what the row knows so far (sh->solve = 1: the solve runs).
SPICEY_FIT_HD void spicey_fit_judge_circuit(const SpiceyFitArgs &A, int32_t c, SpiceyFitShared *sh) {
  const int64_t s0 = (int64_t)c * (1 + 2 * A.nA);
  double *S = A.state + (int64_t)c * spicey_fit_state_doubles(A.nA);
  double *tail = S + (int64_t)A.nA * A.nA + 2 * (int64_t)A.nA;  // F_good, lambda, n_frozen
  const SpiceyFitGoal *G = A.goals + (int64_t)c * A.n_scalar;
  bool evaluable = spicey_fit_ok(A, s0);
  double F = 0.0;
  for (int32_t j = 0; j < A.n_scalar && evaluable; j++) {
    const double x0 = A.x[s0 * A.n_scalar + j];
    if (x0 != x0) { evaluable = false; break; }
    const double r = spicey_fit_resid(G[j], x0);
    F = F + r * r;
  }
  if (!evaluable || F != F) F = INFINITY;
  sh->F = F; sh->maxd = 0.0; sh->minpiv = -1.0; sh->n_clamped = 0; sh->bad = 0; sh->piv = 0;
  sh->accepted = A.first ? spicey_fit_finite(F) : F < tail[0];
  sh->status = 1; sh->solve = 1;
  if (sh->accepted) {
    sh->lam = A.first ? A.lambda0 : tail[1] * A.lam_down;
    sh->n_frozen = 0;  // (counted once the columns are judged)
    if (F <= A.f_tol) { sh->status = 0; sh->solve = 0; }
  } else if (A.first) {
    sh->status = 2; sh->solve = 0; sh->lam = A.lambda0; sh->n_frozen = 0;
  } else {
    sh->lam = tail[1] * A.lam_up;
    sh->n_frozen = (int32_t)tail[2];
    if (!(sh->lam <= A.lam_max)) { sh->status = 5; sh->solve = 0; }
  }
}

// Whether column a of an accepted point is frozen.
SPICEY_FIT_HD int32_t spicey_fit_frozen(const SpiceyFitArgs &A, int32_t c, int32_t a) {
  const int64_t s0 = (int64_t)c * (1 + 2 * A.nA), sp = s0 + 1 + 2 * a;
  if (!spicey_fit_ok(A, sp) || !spicey_fit_ok(A, sp + 1)) return 1;
  const SpiceyFitGoal *G = A.goals + (int64_t)c * A.n_scalar;
  for (int32_t j = 0; j < A.n_scalar; j++) {
    const double r = spicey_fit_resid(G[j], A.x[s0 * A.n_scalar + j]);
    if (!spicey_fit_active(G[j], r)) continue;
    const double d = spicey_fit_jac(A, c, G[j], j, a);
    if (d != d) return 1;
  }
  return 0;
}

// Item idx of an accepted point's normal equations: idx = a1 nA + a2 is A[a1][a2], idx = nA nA + a is b[a].
SPICEY_FIT_HD void spicey_fit_normal(const SpiceyFitArgs &A, int32_t c, const SpiceyFitShared *sh, int32_t idx) {
  const int32_t nA = A.nA;
  const int64_t s0 = (int64_t)c * (1 + 2 * nA);
  double *S = A.state + (int64_t)c * spicey_fit_state_doubles(nA);
  const SpiceyFitGoal *G = A.goals + (int64_t)c * A.n_scalar;
  const bool is_b = idx >= nA * nA;
  const int32_t a1 = is_b ? idx - nA * nA : idx / nA, a2 = is_b ? a1 : idx - a1 * nA;
  double sum = 0.0;
  if (!sh->frz[a1] && !sh->frz[a2]) {
    for (int32_t j = 0; j < A.n_scalar; j++) {
      const double r = spicey_fit_resid(G[j], A.x[s0 * A.n_scalar + j]);
      if (!spicey_fit_active(G[j], r)) continue;
      const double d1 = spicey_fit_jac(A, c, G[j], j, a1);
      const double other = is_b ? r : spicey_fit_jac(A, c, G[j], j, a2);
      sum = sum + d1 * other;
    }
    if (is_b) sum = -sum;
  }
  S[idx] = sum;
}

// What lane 0 does with the pivot of column k.
SPICEY_FIT_HD void spicey_fit_piv_done(const SpiceyFitArgs &A, SpiceyFitShared *sh, int32_t k, const SpiceyPssPiv &p) {
  sh->piv = p.i < 0 ? k : p.i;
  const double v = p.i < 0 ? 0.0 : p.v;
  if (sh->minpiv < 0.0 || v < sh->minpiv) sh->minpiv = v;
  if (!(v >= A.pivot_min)) sh->status = 3;
}

SPICEY_FIT_HD void spicey_fit_row(const SpiceyFitArgs &A, int32_t c, const SpiceyFitShared *sh) {
  const double *tail = A.state + (int64_t)c * spicey_fit_state_doubles(A.nA) + (int64_t)A.nA * A.nA + 2 * (int64_t)A.nA;
  double *dst = A.rows + (int64_t)c * SPICEY_FIT_ROW;
  dst[0] = sh->F; dst[1] = sh->status == 2 ? INFINITY : tail[0]; dst[2] = sh->lam; dst[3] = (double)sh->accepted; dst[4] = (double)sh->status;
  dst[5] = sh->maxd; dst[6] = (double)sh->n_frozen; dst[7] = (double)sh->n_clamped;
  if (sh->status == 0) A.done[c] = 1;
  else if (sh->status >= 2) A.done[c] = sh->status;  // (frozen: no later update touches it)
}

// The update of circuit c.  Ex as in pss_exec.h: ex.par(f) runs f(t) for the threads t = 0 .. ex.T - 1 with a barrier behind it,
// ex.pivot(A, M, k, sh) searches column k's pivot in the first wave (spicey_pss_piv_lane per lane over the row stride nA + 1, the
// lanes met by spicey_pss_piv_meet, spicey_fit_piv_done in lane 0) with a barrier behind it.  Between phases only M, sh and the
// circuit's state carry values.
template <class Ex>
SPICEY_FIT_HD void spicey_fit_update(const SpiceyFitArgs &A, int32_t c, double *M, SpiceyFitShared *sh, Ex &ex) {
  if (A.done[c]) return;  // (the whole workgroup)
  const int32_t nA = A.nA, ld = nA + 1, T = ex.T;
  double *S = A.state + (int64_t)c * spicey_fit_state_doubles(nA);
  double *Sb = S + (int64_t)nA * nA, *Sg = Sb + nA, *tail = Sg + nA;
  double *g = A.g + (int64_t)c * nA;
  ex.par([&](int32_t t) {
    if (t == 0) spicey_fit_judge_circuit(A, c, sh);
  });
  if (sh->accepted) {
    ex.par([&](int32_t t) {
      for (int32_t a = t; a < nA; a += T) sh->frz[a] = spicey_fit_frozen(A, c, a);
    });
    ex.par([&](int32_t t) {
      for (int32_t idx = t; idx < nA * nA + nA; idx += T) spicey_fit_normal(A, c, sh, idx);
      for (int32_t a = t; a < nA; a += T) Sg[a] = g[a];
      if (t == 0) {
        int32_t n = 0;
        for (int32_t a = 0; a < nA; a++) n += sh->frz[a];
        sh->n_frozen = n;
        tail[0] = sh->F; tail[2] = (double)n;
      }
    });
  }
  if (sh->solve) {
    ex.par([&](int32_t t) {
      for (int32_t idx = t; idx < nA * ld; idx += T) {
        const int32_t i = idx / ld, a = idx - i * ld;
        double m = a == nA ? Sb[i] : S[i * nA + a];
        if (a == i) {
          const double extra = sh->lam * m;
          m = m == 0.0 ? 1.0 : m + extra;
        }
        M[idx] = m;
      }
    });
    for (int32_t k = 0; k < nA; k++) {
      ex.pivot(A, M, k, sh);
      if (sh->status == 3) break;
      const int32_t p = sh->piv;
      ex.par([&](int32_t t) {
        if (p != k)
          for (int32_t j = k + t; j < ld; j += T) {
            const double u = M[k * ld + j];
            M[k * ld + j] = M[p * ld + j];
            M[p * ld + j] = u;
          }
      });
      ex.par([&](int32_t t) {
        for (int32_t i = k + 1 + t; i < nA; i += T) M[i * ld + k] = M[i * ld + k] / M[k * ld + k];
      });
      ex.par([&](int32_t t) {
        const int32_t n_cols = nA - k, n_items = (nA - 1 - k) * n_cols;
        for (int32_t idx = t; idx < n_items; idx += T) {
          const int32_t i = k + 1 + idx / n_cols, j = k + 1 + idx % n_cols;
          const double prod = M[i * ld + k] * M[k * ld + j];
          M[i * ld + j] = M[i * ld + j] - prod;
        }
      });
    }
    if (sh->status != 3) {
      for (int32_t k = nA - 1; k >= 0; k--) {
        ex.par([&](int32_t t) {
          const double d = M[k * ld + nA] / M[k * ld + k];  // (row k's right-hand side is final: every thread forms the same d)
          if (t == 0) sh->delta[k] = d;
          for (int32_t i = t; i < k; i += T) {
            const double prod = M[i * ld + k] * d;
            M[i * ld + nA] = M[i * ld + nA] - prod;
          }
        });
      }
      // thread 0: the clamp to max_step and the largest |d|
      ex.par([&](int32_t t) {
        if (t != 0) return;
        double maxd = 0.0;
        for (int32_t a = 0; a < nA; a++) {
          double d = sh->delta[a];
          if (!spicey_fit_finite(d)) { sh->bad = 1; break; }
          d = d > A.max_step ? A.max_step : d < -A.max_step ? -A.max_step : d;
          sh->delta[a] = d;
          if (fabs(d) > maxd) maxd = fabs(d);
        }
        if (sh->bad) sh->status = 4;
        else {
          sh->maxd = maxd;
          if (sh->accepted && maxd <= A.x_tol) sh->status = 0;
        }
      });
    }
  }
  // the last phase: the gains, lambda into the state, the row
  ex.par([&](int32_t t) {
    if (t != 0) return;
    if (sh->status == 1) {
      int32_t n = 0;
      for (int32_t a = 0; a < nA; a++) {
        const double f = 1.0 + sh->delta[a];
        double v = Sg[a] * f;
        const double lo = A.g_lo[(int64_t)c * nA + a], hi = A.g_hi[(int64_t)c * nA + a];
        if (v < lo) { v = lo; n++; }
        else if (v > hi) { v = hi; n++; }
        g[a] = v;
      }
      sh->n_clamped = n;
    } else if (sh->status != 2) {
      for (int32_t a = 0; a < nA; a++) g[a] = Sg[a];
    }
    if (sh->status != 2) tail[1] = sh->lam;
    spicey_fit_row(A, c, sh);
  });
}
