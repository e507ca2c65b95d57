// pss_exec.h — periodic steady state by shooting Newton: the one definition of the design over the STATE of a transient run's
// instances and of the dense Newton update behind one period, used by the kernels of pss.hip and by the CPU harness of
// tests/pss_host (compiled without FMA contraction on both sides, so the two give the same bits).
//
// A handle of n_inst = n_ckt W instances, W = 1 + nX (newton) or 1 (settle); instance c W + j belongs to circuit c, j = 0 is
// nominal, j = 1 + a has state entry a perturbed.  The state vector of one circuit is x = [C_vprev | L_iprev | D_vdprev],
// nX = nC + nL + nD; S_ison is carried, not differentiated.
//
// The design.  One thread per (instance s, entry a) writes into the run's own state arrays
//   s[c][j][a] = base[c][a], and for j == 1 + a the value sp = base[c][a] + rel_step max(|base[c][a]|, scale_kind(a))
//   h_eff[c][a] = sp - base[c][a]                     (the representable difference; written by the thread of j == 1 + a)
// — a product, then a sum, then a difference —; the thread of entry 0 gives its instance base_on[c] as S_ison.  scale is v_scale
// for C and D entries and i_scale for L entries.  With perturb = 0 every instance gets the base alone and h_eff is left as it is.
//
// The update.  One workgroup of SPICEY_PSS_THREADS per circuit, every phase followed by a barrier; a circuit whose done[c] is
// set is left untouched.  e_j: the end state of instance c W + j, e0 the nominal's, r = e0 - base.
//   judge      thread 0: res = max_a |r_a| / (reltol max(|base_a|, |e0_a|) + abstol_kind(a)), a_res the lowest entry at the
//              maximum; n_switch_mismatch = #{k : S_ison(nominal)[k] != base_on[c][k]}; n_pert_switch_diff = the perturbed
//              instances whose end S_ison differs from the nominal's; the instances' run statuses (ist, null: all 0).
//   matrix     M[i][a] = (i == a ? 1 : 0) - (e_{1+a}[i] - e0[i]) / h_eff[a], column nX = r; row stride nX + 1 doubles.
//   eliminate  k = 0 .. nX - 1: the pivot row is the LOWEST i >= k with the largest |M[i][k]|; |pivot| < 1e-12 stops with
//              status 3; rows k and pivot are exchanged; M[i][k] = M[i][k] / M[k][k] for i > k; M[i][j] = M[i][j] - M[i][k] M[k][j]
//              for i > k, j > k, the right-hand side included — each quotient, product and difference rounded on its own.
//   solve      k = nX - 1 .. 0: d_k = rhs_k / M[k][k]; rhs_i = rhs_i - M[i][k] d_k for i < k.
//   answer     base[c][a] = base[c][a] + damping d_a (one product, one sum), base_on[c] = the nominal's end S_ison.
// Status, the first that applies: 2 the nominal's run was singular (ist > 0); 5 the nominal was stopped by another circuit's
// failure (ist < 0); 4 a base or nominal end entry is not finite; 0 converged (res <= 1 and no switch mismatch: done[c] is set,
// the base stays); settle moves (base = e0, d = r, status 1); 4 a perturbed instance's run was singular; 5 one was stopped by
// another circuit's failure; 4 a matrix entry is not finite; 3 a pivot below 1e-12; 4 a d that is not finite; else 1: moved, not
// yet converged.  With a status >= 2 the base, base_on and d are left as they are and done[c] takes the status: the circuit is frozen.
//   rows [n_ckt][8] = {res, step, n_switch_mismatch, status, a_res, min |pivot|, n_pert_switch_diff, converged}
// step = max_a |d_a| / (reltol |base_a| + abstol_kind(a)) on the base before the move (0 where nothing moved); min |pivot| over
// the pivots taken (-1 when none was).  Every field is a max, a count or a copy: nothing depends on the thread count.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/spicey_hip.h"

#if defined(__HIPCC__)
#define SPICEY_PSS_HD __host__ __device__ __forceinline__
#else
#define SPICEY_PSS_HD inline
#endif

#define SPICEY_PSS_MAX_NX 128    // states of one circuit the Newton update takes (its matrix lives in LDS)
#define SPICEY_PSS_THREADS 256   // the update's workgroup; the design's too
#define SPICEY_PSS_LANES 64      // the wave that searches the pivot
#define SPICEY_PSS_PIVOT_MIN 1e-12

// A validated call with the buffers it runs on (pss.h: spicey_pss_judge).  ist lies in the workspace.
struct SpiceyPssArgs {
  double *base;          // [n_ckt][nX]
  int32_t *base_on;      // [n_ckt][nS]
  double *h_eff;         // [n_ckt][nX]      newton
  double *Cv, *Li, *Dv;  // [n_inst][n<kind>] the run's state arrays
  int32_t *Son;          // [n_inst][nS]
  double *delta;         // [n_ckt][nX]      or null
  double *rows;          // [n_ckt][8]
  int32_t *done;         // [n_ckt]
  const int32_t *ist;    // [n_inst] the instances' run statuses, or null
  double damping, reltol, vabstol, iabstol, rel_step, v_scale, i_scale;
  int32_t n_ckt, nC, nL, nD, nS, method, perturb, pad;
};

SPICEY_PSS_HD int32_t spicey_pss_nx(const SpiceyPssArgs &A) { return A.nC + A.nL + A.nD; }
SPICEY_PSS_HD int32_t spicey_pss_w(const SpiceyPssArgs &A) { return A.method == SPICEY_PSS_SETTLE ? 1 : 1 + spicey_pss_nx(A); }
SPICEY_PSS_HD bool spicey_pss_is_l(const SpiceyPssArgs &A, int32_t a) { return a >= A.nC && a < A.nC + A.nL; }
// Where entry a of instance s lives.
SPICEY_PSS_HD double *spicey_pss_entry(const SpiceyPssArgs &A, int64_t s, int32_t a) {
  if (a < A.nC) return A.Cv + s * A.nC + a;
  if (a < A.nC + A.nL) return A.Li + s * A.nL + (a - A.nC);
  return A.Dv + s * A.nD + (a - A.nC - A.nL);
}
SPICEY_PSS_HD bool spicey_pss_finite(double v) { return v - v == 0.0; }

// Thread idx = s * nX + a of the design kernel.
SPICEY_PSS_HD void spicey_pss_design(const SpiceyPssArgs &A, int64_t idx) {
  const int32_t nX = spicey_pss_nx(A), W = spicey_pss_w(A);
  const int64_t s = idx / nX;
  const int32_t a = (int32_t)(idx - s * nX);
  const int64_t c = s / W;
  const int32_t j = (int32_t)(s - c * W);
  const double b = A.base[c * nX + a];
  double v = b;
  if (A.perturb && j == 1 + a) {
    const double m = fmax(fabs(b), spicey_pss_is_l(A, a) ? A.i_scale : A.v_scale);
    const double step = A.rel_step * m;
    v = b + step;
    A.h_eff[c * nX + a] = v - b;
  }
  *spicey_pss_entry(A, s, a) = v;
  if (a == 0)
    for (int32_t k = 0; k < A.nS; k++) A.Son[s * A.nS + k] = A.base_on[c * A.nS + k];
}

// What the phases of one circuit's update share besides the matrix (static LDS on the device).
struct SpiceyPssShared {
  double delta[SPICEY_PSS_MAX_NX];
  double res, step, minpiv;
  int32_t a_res, n_mis, n_pert, status, piv, bad, go, pad;
};

// The pivot search: what one lane brings, and how two meet (the larger |value|; of equal ones the lower row).
struct SpiceyPssPiv { double v; int32_t i; };
SPICEY_PSS_HD SpiceyPssPiv spicey_pss_piv_lane(const double *M, int32_t nX, int32_t k, int32_t lane) {
  SpiceyPssPiv p{-1.0, -1};
  for (int32_t i = k + lane; i < nX; i += SPICEY_PSS_LANES) {
    const double v = fabs(M[(int64_t)i * (nX + 1) + k]);
    if (v > p.v) { p.v = v; p.i = i; }
  }
  return p;
}
SPICEY_PSS_HD void spicey_pss_piv_meet(SpiceyPssPiv *p, const SpiceyPssPiv &q) {
  if (q.i >= 0 && (p->i < 0 || q.v > p->v || (q.v == p->v && q.i < p->i))) *p = q;
}
// What lane 0 does with the pivot of column k.  (no lane found a row: every entry of the column is NaN)
SPICEY_PSS_HD void spicey_pss_piv_done(SpiceyPssShared *sh, int32_t k, const SpiceyPssPiv &p) {
  sh->piv = p.i < 0 ? k : p.i;
  const double v = p.i < 0 ? 0.0 : p.v;
  if (sh->minpiv < 0.0 || v < sh->minpiv) sh->minpiv = v;
  if (!(v >= SPICEY_PSS_PIVOT_MIN)) sh->status = 3;
}

// Thread 0's judgement of circuit c before any matrix: the row's counts and residual, and the status as far as it is known
// (sh->go = 1: the elimination runs).
SPICEY_PSS_HD void spicey_pss_judge_circuit(const SpiceyPssArgs &A, int32_t c, SpiceyPssShared *sh) {
  const int32_t nX = spicey_pss_nx(A), W = spicey_pss_w(A);
  const int64_t s0 = (int64_t)c * W;
  sh->res = 0.0; sh->step = 0.0; sh->minpiv = -1.0;
  sh->a_res = 0; sh->n_mis = 0; sh->n_pert = 0; sh->status = 1; sh->piv = 0; sh->bad = 0; sh->go = 0;
  bool bad0 = false;
  for (int32_t a = 0; a < nX; a++) {
    const double b = A.base[(int64_t)c * nX + a], e = *spicey_pss_entry(A, s0, a);
    if (!spicey_pss_finite(b) || !spicey_pss_finite(e)) { bad0 = true; continue; }
    const double r = e - b;
    const double tol = A.reltol * fmax(fabs(b), fabs(e)) + (spicey_pss_is_l(A, a) ? A.iabstol : A.vabstol);
    const double q = fabs(r) / tol;
    if (q > sh->res) { sh->res = q; sh->a_res = a; }
  }
  for (int32_t k = 0; k < A.nS; k++) sh->n_mis += A.Son[s0 * A.nS + k] != A.base_on[(int64_t)c * A.nS + k];
  int32_t pert_sing = 0, pert_stop = 0;
  for (int32_t j = 1; j < W; j++) {
    bool diff = false;
    for (int32_t k = 0; k < A.nS; k++) diff = diff || A.Son[(s0 + j) * A.nS + k] != A.Son[s0 * A.nS + k];
    sh->n_pert += diff;
    if (A.ist) { pert_sing += A.ist[s0 + j] > 0; pert_stop += A.ist[s0 + j] < 0; }
  }
  const int32_t ist0 = A.ist ? A.ist[s0] : 0;
  if (ist0 > 0) sh->status = 2;
  else if (ist0 < 0) sh->status = 5;
  else if (bad0) sh->status = 4;
  else if (sh->res <= 1.0 && sh->n_mis == 0) sh->status = 0;
  else if (A.method == SPICEY_PSS_SETTLE) sh->status = 1;
  else if (pert_sing) sh->status = 4;
  else if (pert_stop) sh->status = 5;
  else sh->go = 1;
}

// Item idx = i (nX + 1) + a of the matrix of circuit c.
SPICEY_PSS_HD void spicey_pss_matrix(const SpiceyPssArgs &A, int32_t c, double *M, SpiceyPssShared *sh, int32_t idx) {
  const int32_t nX = spicey_pss_nx(A), ld = nX + 1;
  const int32_t i = idx / ld, a = idx - i * ld;
  const int64_t s0 = (int64_t)c * (1 + nX);
  const double e0 = *spicey_pss_entry(A, s0, i);
  double m;
  if (a == nX) m = e0 - A.base[(int64_t)c * nX + i];
  else {
    const double d = *spicey_pss_entry(A, s0 + 1 + a, i) - e0;
    const double q = d / A.h_eff[(int64_t)c * nX + a];
    m = (i == a ? 1.0 : 0.0) - q;
  }
  if (!spicey_pss_finite(m)) sh->bad = 1;  // (every writer writes the same value)
  M[idx] = m;
}

// d of entry a once it is known: the solution, or with settle the residual (any nX: nothing of it is kept in sh).
SPICEY_PSS_HD double spicey_pss_d(const SpiceyPssArgs &A, int32_t c, const SpiceyPssShared *sh, int32_t a) {
  if (A.method != SPICEY_PSS_SETTLE) return sh->delta[a];
  return *spicey_pss_entry(A, (int64_t)c, a) - A.base[(int64_t)c * spicey_pss_nx(A) + a];
}

// Thread 0's scaled max-norm of d on the base before the move.
SPICEY_PSS_HD void spicey_pss_step_norm(const SpiceyPssArgs &A, int32_t c, SpiceyPssShared *sh) {
  const int32_t nX = spicey_pss_nx(A);
  double step = 0.0;
  for (int32_t a = 0; a < nX; a++) {
    const double d = spicey_pss_d(A, c, sh, a);
    if (!spicey_pss_finite(d)) { sh->bad = 2; return; }
    const double tol = A.reltol * fabs(A.base[(int64_t)c * nX + a]) + (spicey_pss_is_l(A, a) ? A.iabstol : A.vabstol);
    const double q = fabs(d) / tol;
    if (q > step) step = q;
  }
  sh->step = step;
}

SPICEY_PSS_HD void spicey_pss_row(const SpiceyPssArgs &A, int32_t c, const SpiceyPssShared *sh) {
  double *dst = A.rows + (int64_t)c * SPICEY_PSS_ROW;
  dst[0] = sh->res; dst[1] = sh->step; dst[2] = (double)sh->n_mis; dst[3] = (double)sh->status; dst[4] = (double)sh->a_res;
  dst[5] = sh->minpiv; dst[6] = (double)sh->n_pert; dst[7] = sh->status == 0 ? 1.0 : 0.0;
  if (sh->status == 0) A.done[c] = 1;
  else if (sh->status >= 2) A.done[c] = sh->status;  // (frozen: no later update touches it)
}

// The update of circuit c.  Ex runs a phase in every thread and puts a barrier behind it — ex.par(f): f(t) for the threads
// t = 0 .. ex.T - 1 — and searches a pivot in its first wave — ex.pivot(M, nX, k, sh): spicey_pss_piv_lane per lane, the lanes
// met by spicey_pss_piv_meet, spicey_pss_piv_done in lane 0, a barrier behind it.  Between phases only M and sh carry values.
template <class Ex>
SPICEY_PSS_HD void spicey_pss_update(const SpiceyPssArgs &A, int32_t c, double *M, SpiceyPssShared *sh, Ex &ex) {
  if (A.done[c]) return;  // (the whole workgroup)
  const int32_t nX = spicey_pss_nx(A), ld = nX + 1, T = ex.T;
  const int64_t s0 = (int64_t)c * spicey_pss_w(A);
  ex.par([&](int32_t t) {
    if (t == 0) spicey_pss_judge_circuit(A, c, sh);
  });
  if (sh->go) {
    ex.par([&](int32_t t) {
      for (int32_t idx = t; idx < nX * ld; idx += T) spicey_pss_matrix(A, c, M, sh, idx);
    });
    if (sh->bad) {
      ex.par([&](int32_t t) {
        if (t == 0) { sh->status = 4; sh->go = 0; }
      });
    }
  }
  if (sh->go) {
    for (int32_t k = 0; k < nX; k++) {
      ex.pivot(M, nX, k, sh);
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
        for (int32_t i = k + 1 + t; i < nX; i += T) M[i * ld + k] = M[i * ld + k] / M[k * ld + k];
      });
      ex.par([&](int32_t t) {
        const int32_t n_cols = nX - k, n_items = (nX - 1 - k) * n_cols;
        for (int32_t idx = t; idx < n_items; idx += T) {
          const int32_t i = k + 1 + idx / n_cols, j = k + 1 + idx % n_cols;
          const double prod = M[i * ld + k] * M[k * ld + j];
          M[i * ld + j] = M[i * ld + j] - prod;
        }
      });
    }
    if (sh->status != 3) {
      for (int32_t k = nX - 1; k >= 0; k--) {
        ex.par([&](int32_t t) {
          const double d = M[k * ld + nX] / M[k * ld + k];  // (row k's right-hand side is final: every thread forms the same d)
          if (t == 0) sh->delta[k] = d;
          for (int32_t i = t; i < k; i += T) {
            const double prod = M[i * ld + k] * d;
            M[i * ld + nX] = M[i * ld + nX] - prod;
          }
        });
      }
    }
  }
  // (a phase never writes what decides, between the barrier before it and itself, whether a thread enters it: a d that is
  // not finite is noted in sh->bad and becomes the status in the last phase)
  if (sh->status == 1) {
    ex.par([&](int32_t t) {
      if (t == 0) spicey_pss_step_norm(A, c, sh);
    });
  }
  if (sh->status == 1 && sh->bad == 0) {
    ex.par([&](int32_t t) {
      for (int32_t a = t; a < nX; a += T) {
        const double d = spicey_pss_d(A, c, sh, a);
        double *b = A.base + (int64_t)c * nX + a;
        if (A.method == SPICEY_PSS_SETTLE) *b = *spicey_pss_entry(A, s0, a);
        else {
          const double move = A.damping * d;
          *b = *b + move;
        }
        if (A.delta) A.delta[(int64_t)c * nX + a] = d;
      }
      for (int32_t k = t; k < A.nS; k += T) A.base_on[(int64_t)c * A.nS + k] = A.Son[s0 * A.nS + k];
    });
  }
  ex.par([&](int32_t t) {
    if (t == 0) {
      if (sh->bad == 2) sh->status = 4;
      spicey_pss_row(A, c, sh);
    }
  });
}
