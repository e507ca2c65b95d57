// ac_exact_exec.h — the reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3; device code,
// host-compilable).
//
// One workgroup solves one (instance, frequency) slot the way the reference does it, operation for operation, so that
// every double it produces is the reference's:
//   buildLinearSystemForAC    simulateAC.ts:25-62     a zero complex A | b; every entry is the sum of its contributions
//                                                     from (+0, +0) in the reference's element order (R, C, L, V;
//                                                     ac_exact_plan.cpp lists them per entry) by Complex.add / sub on
//                                                     both components, one thread per entry
//   solveComplex              lib/math/solveComplex.ts:4-73   dense Gaussian elimination with partial pivoting on the
//                                                     augmented matrix: first strict maximum of |a_ik| (V8's Math.hypot),
//                                                     `vmax < EPS` = singular, row swap (a permutation), multipliers
//                                                     f = a_ik.div(pivot) (Complex.div: |pivot|^2 < EPS throws), rows with
//                                                     |f| < EPS skipped (:46), row updates for j = k..n in parallel, back
//                                                     substitution row by row, every term, in ascending j
//   recording                 simulateAC.ts:84-126    node voltages; currents of R, C, L (Y.mul(v1.sub(v2))) and V
// The executable specification is the checker spicey_ref_ac.c.  The including translation unit must not contract a * b + c
// into FMAs (ac_exact.hip: `#pragma clang fp contract(off)`; the CPU test harness: -ffp-contract=off), and its sqrt must
// be correctly rounded.
//
// Exec (as for exact_exec.h): threads(), phase(tag, f) = f(tid) for every thread, then a workgroup barrier;
// atomic_add(int32_t *, int) on workgroup-local counters; argmax(count, get, &v, &i) = over j in [0, count) the largest
// get(j) that is not NaN, lowest j among equals (v = -1, i = INT_MAX when there is none), known to every thread on return.
// Control flow outside phases is workgroup-uniform.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ac_exact_plan.h"
#include "ac_exec.h"

#define SPICEY_AC_EXACT_TWO_PI (2 * 3.141592653589793)  // simulateAC.ts: 2 * Math.PI

struct SpiceyAcExactRun {
  const double *R_inv, *C_val, *L_val;  // [n_inst][n<kind>]; R_inv = 1.0 / R formed on the host (the reference's own
                                        // correctly rounded quotient, simulateAC.ts:39-41)
  const double *freqs;                  // [n_freq]
  const double *vph;                    // [n_inst][nV][2] source phasors
  double *out_v;                        // [n_inst][n_freq][nOut][2]
  double *out_i;                        // [n_inst][n_freq][nR+nC+nL+nV][2] or null
  SpiceyCx *gW;                         // [workgroups of a launch][ws_cx] global slab, or null when the workspace is in LDS
  int32_t *status;                      // [n_inst * n_freq] 0 ok, 1 singular, 5 complex divide by ~0
  int64_t *skipped;                     // [n_inst * n_freq] nonzero multipliers the |f| < EPS test dropped, or null
  int64_t n_freq;
  int32_t n_inst;
};

// V8's Math.hypot for two arguments (builtins math.tq, what Complex.abs runs): NaN / Inf rules, scaling by the maximum,
// Kahan-compensated sum of squares, sqrt(sum) * max
SPICEY_HD double spicey_v8_hypot(double x, double y) {
  const double ax = fabs(x), ay = fabs(y);
  if (x != x || y != y) return (isinf(x) || isinf(y)) ? INFINITY : NAN;
  double mx = 0.0;
  if (ax > mx) mx = ax;
  if (ay > mx) mx = ay;
  if (mx == INFINITY) return INFINITY;
  if (mx == 0.0) return 0.0;
  double sum = 0.0, comp = 0.0;
  const double a0 = ax / mx, s0 = a0 * a0 - comp, p0 = sum + s0;
  comp = (p0 - sum) - s0;
  sum = p0;
  const double a1 = ay / mx, s1 = a1 * a1 - comp, p1 = sum + s1;
  sum = p1;
  return sqrt(sum) * mx;
}
SPICEY_HD double spicey_v8_abs(SpiceyCx z) { return spicey_v8_hypot(z.re, z.im); }

// Complex.div (Complex.ts:38-45) once its guard has passed: d = b.re * b.re + b.im * b.im, d >= EPS (or NaN)
SPICEY_HD SpiceyCx spicey_ac_exact_div(SpiceyCx a, SpiceyCx b, double d) {
  return SpiceyCx{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
SPICEY_HD double spicey_ac_exact_norm2(SpiceyCx b) { return b.re * b.re + b.im * b.im; }

// The inductor's admittance (simulateAC.ts:47-55): denom = (0, wL); Y = 0 when |denom| < EPS, else Complex(1, 0).div(denom),
// which refuses |denom|^2 < EPS (bad = true)
SPICEY_HD SpiceyCx spicey_ac_exact_ind(double wl, bool &bad) {
  const SpiceyCx denom{0.0, wl};
  bad = false;
  if (spicey_v8_abs(denom) < SPICEY_EPS) return SpiceyCx{0.0, 0.0};
  const double d = spicey_ac_exact_norm2(denom);
  if (d < SPICEY_EPS) { bad = true; return SpiceyCx{0.0, 0.0}; }
  return spicey_ac_exact_div(SpiceyCx{1.0, 0.0}, denom, d);
}

// One (instance, frequency) slot.  ws = its workspace (P.ws_cx complex entries; LDS or its slab of the global buffer);
// scal = 4 workgroup-local counters: [0, 1] active rows of the pivot step (by parity: a counter is cleared two steps
// after it was read), [2] skipped multipliers, [3] error code.
template <class Exec>
SPICEY_HD void spicey_ac_exact_solve(Exec &ex, const SpiceyAcExactProg &P, const SpiceyAcExactRun &R, SpiceyCx *ws, int32_t *scal, int64_t slot) {
  const int T = ex.threads(), n = P.n, ld = P.ld;
  const size_t inst = (size_t)(slot / R.n_freq);
  const double w = SPICEY_AC_EXACT_TWO_PI * R.freqs[slot % R.n_freq];  // twoPi * f * C = (twoPi * f) * C
  SpiceyCx *A = ws + P.oA, *x = ws + P.ox, *q = ws + P.oq, *act_f = ws + P.of;
  int32_t *perm = (int32_t *)(ws + P.operm), *act_r = (int32_t *)(ws + P.oact);
  const double *Rinv = R.R_inv + inst * P.nR, *Cv = R.C_val + inst * P.nC, *Lv = R.L_val + inst * P.nL;
  const int n_q = P.nR + P.nC + P.nL + P.nV;
  auto volt = [&](int node) { return node == 0 ? SpiceyCx{0.0, 0.0} : x[node - 1]; };
  ex.phase(SPICEY_PH_PRO, [&](int tid) {
    if (tid == 0) { scal[0] = 0; scal[1] = 0; scal[2] = 0; scal[3] = 0; }
  });
  // ---- the frequency's quantities (one thread per element), a zero A | b and the identity row order
  ex.phase(SPICEY_PH_B, [&](int tid) {
    for (int e = tid; e < n_q; e += T) {
      int i = e;
      if (i < P.nR) { q[P.qR + i] = SpiceyCx{Rinv[i], 0.0}; continue; }
      i -= P.nR;
      if (i < P.nC) { q[P.qC + i] = SpiceyCx{0.0, w * Cv[i]}; continue; }
      i -= P.nC;
      if (i < P.nL) {
        bool bad;
        q[P.qL + i] = spicey_ac_exact_ind(w * Lv[i], bad);
        if (bad) scal[3] = SPICEY_ERR_COMPLEX_DIV_CODE;  // (every writer writes the same value)
        continue;
      }
      i -= P.nL;
      const double *ph = R.vph + (inst * P.nV + i) * 2;
      q[P.qV + i] = SpiceyCx{ph[0], ph[1]};
    }
    if (tid == 0) q[P.qOne] = SpiceyCx{1.0, 0.0};
    for (size_t i = (size_t)tid; i < (size_t)n * (size_t)ld; i += (size_t)T) A[i] = SpiceyCx{0.0, 0.0};
    for (int i = tid; i < n; i += T) perm[i] = i;
  });
  // ---- stamps: every entry sums its contributions in the reference's order
  ex.phase(SPICEY_PH_B, [&](int tid) {
    for (int e = tid; e < P.nEnt; e += T) {
      SpiceyCx s{0.0, 0.0};
      for (uint32_t c = P.ent_ptr[e]; c < P.ent_ptr[e + 1]; c++) {
        const uint32_t wd = P.ent_src[c];
        const SpiceyCx v = q[wd & ~SPICEY_AC_EXACT_SUB];
        s = (wd & SPICEY_AC_EXACT_SUB) ? cx_sub(s, v) : cx_add(s, v);
      }
      A[P.ent_pos[e]] = s;
    }
  });
  int code = scal[3];  // (an inductor the reference refuses while it builds the system)
  // ---- forward elimination (solveComplex.ts:15-53)
  for (int k = 0; k < n && code == 0; k++) {
    double bv;
    int bi;
    ex.argmax(n - k, [&](int j) { return spicey_v8_abs(A[(size_t)perm[k + j] * ld + k]); }, bv, bi);
    const double akk = spicey_v8_abs(A[(size_t)perm[k] * ld + k]);
    if (akk != akk) { bv = akk; bi = 0; }  // (a NaN |a_kk|: no |a_ik| > NaN, the reference keeps row k)
    if (bv < SPICEY_EPS) { code = SPICEY_ERR_SINGULAR; break; }
    const int imax = k + bi;
    const int pr = perm[imax], kr = perm[k];
    const SpiceyCx *prow = A + (size_t)pr * ld;
    const SpiceyCx pivot = prow[k];
    const double d = spicey_ac_exact_norm2(pivot);
    if (k < n - 1 && d < SPICEY_EPS) { code = SPICEY_ERR_COMPLEX_DIV_CODE; break; }  // the first row's a_ik.div(pivot) throws
    int32_t *na_k = scal + (k & 1);
    ex.phase(SPICEY_PH_U0, [&](int tid) {
      if (tid == 0) scal[(k + 1) & 1] = 0;
      for (int i = k + 1 + tid; i < n; i += T) {
        const int r = i == imax ? kr : perm[i];
        const SpiceyCx f = spicey_ac_exact_div(A[(size_t)r * ld + k], pivot, d);
        if (spicey_v8_abs(f) < SPICEY_EPS) {  // solveComplex.ts:46
          if (f.re != 0.0 || f.im != 0.0) ex.atomic_add(&scal[2], 1);
          continue;
        }
        const int a = ex.atomic_add(na_k, 1);
        act_r[a] = r;
        act_f[a] = f;
      }
    });
    const int na = *na_k;
    // the row swap (after every thread has read pr, kr) and row[j] = row[j].sub(f.mul(prow[j])), j = k + 1 .. n (column k
    // of the rows below is never read again); a wave per row
    if (na > 0 || imax != k)
      ex.phase(SPICEY_PH_U0, [&](int tid) {
        if (tid == 0) {
          perm[k] = pr;
          perm[imax] = kr;
        }
        const int nw = (T + 63) >> 6, wv = tid >> 6, lane = tid & 63;
        for (int a = wv; a < na; a += nw) {
          SpiceyCx *row = A + (size_t)act_r[a] * ld;
          const SpiceyCx f = act_f[a];
          for (int j = k + 1 + lane; j <= n; j += 64) row[j] = cx_sub(row[j], cx_mul(f, prow[j]));
        }
      });
  }
  // ---- back substitution (solveComplex.ts:56-72): s = b_i; s = s.sub(a_ij.mul(x_j)) for j = i+1 .. n-1 ascending, every
  //      term; x_i = s.div(a_ii), which throws for |a_ii|^2 < EPS (only the last pivot can still do so here)
  if (code == 0) {
    ex.phase(SPICEY_PH_K0, [&](int tid) {
      if (tid != 0) return;
      for (int i = n - 1; i >= 0; i--) {
        const SpiceyCx *row = A + (size_t)perm[i] * ld;
        SpiceyCx s = row[n];
        for (int j = i + 1; j < n; j++) s = cx_sub(s, cx_mul(row[j], x[j]));
        const double dd = spicey_ac_exact_norm2(row[i]);
        if (dd < SPICEY_EPS) { scal[3] = SPICEY_ERR_COMPLEX_DIV_CODE; return; }
        x[i] = spicey_ac_exact_div(s, row[i], dd);
      }
    });
    code = scal[3];
  }
  // ---- recording (simulateAC.ts:84-126)
  if (code == 0)
    ex.phase(SPICEY_PH_Z, [&](int tid) {
      double *ov = R.out_v + (size_t)slot * P.nOut * 2;
      for (int i = tid; i < P.nOut; i += T) {
        const SpiceyCx v = volt(P.out_nodes[i]);
        ov[2 * i] = v.re;
        ov[2 * i + 1] = v.im;
      }
      if (!R.out_i) return;
      double *oi = R.out_i + (size_t)slot * P.nCur * 2;
      for (int e = tid; e < P.nCur; e += T) {
        int i = e;
        SpiceyCx cur;
        if (i < P.nR) {
          cur = cx_mul(SpiceyCx{Rinv[i], 0.0}, cx_sub(volt(P.R_nd[2 * i]), volt(P.R_nd[2 * i + 1])));
        } else if ((i -= P.nR) < P.nC) {
          cur = cx_mul(SpiceyCx{0.0, w * Cv[i]}, cx_sub(volt(P.C_nd[2 * i]), volt(P.C_nd[2 * i + 1])));
        } else if ((i -= P.nC) < P.nL) {
          bool bad;
          cur = cx_mul(spicey_ac_exact_ind(w * Lv[i], bad), cx_sub(volt(P.L_nd[2 * i]), volt(P.L_nd[2 * i + 1])));
        } else {
          cur = x[P.nN + (i - P.nL)];
        }
        oi[2 * e] = cur.re;
        oi[2 * e + 1] = cur.im;
      }
    });
  ex.phase(SPICEY_PH_Z, [&](int tid) {
    if (tid != 0) return;
    R.status[slot] = code;
    if (R.skipped) R.skipped[slot] = scal[2];
  });
}
