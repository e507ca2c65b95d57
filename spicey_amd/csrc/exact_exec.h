// exact_exec.h — the reference-order transient engine (SpiceyOptions.interpreter = 3; device code, host-compilable).
//
// One workgroup runs one instance's whole `for step … for iter …` nest the way the reference does it, operation for
// operation, so that every double it produces is the reference's:
//   stampAllElementsAtTime    simulateTRAN.ts:25-102   a fresh dense A | b per iteration; every entry is the sum of its
//                                                      contributions from +0.0 in the reference's element order (R, C, L,
//                                                      S, V, D; exact_plan.cpp lists them per entry), one thread per entry
//   solveReal                 lib/math/solveReal.ts:3-73   dense Gaussian elimination with partial pivoting on the
//                                                      augmented matrix: first strict maximum of |a_ik|, `vmax < EPS` =
//                                                      singular, row swap (a permutation), multipliers f = a_ik / pivot,
//                                                      rows with |f| < EPS skipped (:46), row updates for j = k..n in
//                                                      parallel, back substitution row by row in ascending j
//   switch iteration, recording, state update   simulateTRAN.ts:108-128, :146-237
// The executable specification is the checker spicey_ref.c; Math.exp is fdlibm's __ieee754_exp (what V8 runs), restated below.
// The including translation unit must not contract a * b + c into FMAs (exact.hip: `#pragma clang fp contract(off)`;
// the CPU test harness: -ffp-contract=off).
//
// Exec (same arrangement as tran_exec.h / ac_exec.h): threads(), phase(tag, f) = f(tid) for every thread, then a workgroup
// barrier; atomic_add(int32_t *, int) on workgroup-local counters; argmax(count, get, &v, &i) = over j in [0, count) the
// largest get(j) that is not NaN, lowest j among equals (v = -1, i = INT_MAX when there is none), known to every thread
// on return.  Control flow outside phases is workgroup-uniform.
#pragma once
#include <math.h>
#include <stdint.h>

#include "exact_plan.h"
#include "program.h"
#include "tran_common.h"


// fdlibm e_exp.c (Sun Microsystems, 1993/2004), as V8 runs it for Math.exp: argument reduction by ln2 hi/lo, degree-5
// polynomial in r * r, scaling by 2^k.
SPICEY_HD double spicey_exact_bits_to_double(uint64_t b) {
  double x;
  __builtin_memcpy(&x, &b, 8);
  return x;
}
SPICEY_HD double spicey_fdlibm_exp(double x) {
  const double one = 1.0, huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, o_threshold = 7.09782712893383973096e+02,
               u_threshold = -7.45133219101941108420e+02, ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
               invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
               P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08, E = 2.718281828459045;
  double y, hi = 0.0, lo = 0.0, c, t, twopk;
  int32_t k = 0;
  uint64_t bits;
  __builtin_memcpy(&bits, &x, 8);
  uint32_t hx = (uint32_t)(bits >> 32);
  const uint32_t lx = (uint32_t)bits;
  const int32_t xsb = (int32_t)((hx >> 31) & 1);
  hx &= 0x7fffffff;
  if (hx >= 0x40862E42) { /* |x| >= 709.78... */
    if (hx >= 0x7ff00000) {
      if (((hx & 0xfffff) | lx) != 0) return x + x; /* NaN */
      return (xsb == 0) ? x : 0.0;                    /* exp(+-inf) = {inf, 0} */
    }
    if (x > o_threshold) return huge * huge;
    if (x < u_threshold) return twom1000 * twom1000;
  }
  if (hx > 0x3fd62e42) {   /* |x| > 0.5 ln2 */
    if (hx < 0x3FF0A2B2) { /* and |x| < 1.5 ln2 */
      if (x == 1.0) return E;
      hi = x - (xsb ? -ln2HI : ln2HI);
      lo = xsb ? -ln2LO : ln2LO;
      k = 1 - xsb - xsb;
    } else {
      k = (int32_t)(invln2 * x + (xsb ? -0.5 : 0.5));
      t = k;
      hi = x - t * ln2HI;
      lo = t * ln2LO;
    }
    x = hi - lo;
  } else if (hx < 0x3e300000) { /* |x| < 2**-28 */
    if (huge + x > one) return one + x;
  } else {
    k = 0;
  }
  t = x * x;
  if (k >= -1021)
    bits = (uint64_t)(uint32_t)(0x3ff00000 + (int32_t)((uint32_t)k << 20)) << 32;
  else
    bits = (uint64_t)(uint32_t)(0x3ff00000 + (int32_t)((uint32_t)(k + 1000) << 20)) << 32;
  twopk = spicey_exact_bits_to_double(bits);
  c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return one - ((x * c) / (c - 2.0) - x);
  y = one - ((lo - (x * c) / (2.0 - c)) - hi);
  if (k >= -1021) {
    if (k == 1024) return y * 2.0 * 8.98846567431158e+307; /* 0x1p1023 */
    return y * twopk;
  }
  return y * twopk * twom1000;
}

// Math.max(a, b): NaN if either is NaN
SPICEY_HD double spicey_exact_max(double a, double b) {
  if (a != a || b != b) return spicey_exact_bits_to_double(0x7ff8000000000000ull);
  return a > b ? a : b;
}
SPICEY_HD bool spicey_exact_is_neg_zero(double s) { return s == 0.0 && signbit(s); }

// One instance (`inst`), one run of steps + 1 points.  ws = the instance's workspace (P.ws_doubles doubles; LDS or its
// slab of the global buffer); scal = 8 workgroup-local counters.  Results, state and diagnostics go where SpiceyRun says;
// status[wg * 4 ..] = {code, inst, step, iter}.
template <class Exec>
SPICEY_HD void spicey_exact_run(Exec &ex, const SpiceyExactProg &P, const SpiceyRun &R, double *ws, int32_t *scal, int inst, int wg) {
  const int T = ex.threads(), n = P.n, ld = P.ld, mw = P.mw;
  const size_t in = (size_t)inst;
  double *A = ws + P.oA, *x = ws + P.ox, *q = ws + P.oq, *vdlin = ws + P.ovdlin, *act_f = ws + P.oact_f;
  int32_t *perm = (int32_t *)(ws + P.operm), *act_r = (int32_t *)(ws + P.oact_r);
  uint32_t *mask = (uint32_t *)(ws + P.omask);
  const double *Rv = R.R_val + in * P.nR, *Cv = R.C_val + in * P.nC, *Lv = R.L_val + in * P.nL;
  const double *Ron = R.S_ron + in * P.nS, *Roff = R.S_roff + in * P.nS, *Von = R.S_von + in * P.nS, *Voff = R.S_voff + in * P.nS;
  const double *Dis = R.D_is + in * P.nD, *Dn = R.D_n + in * P.nD;
  double *vprev = R.C_vprev + in * P.nC, *iprev = R.L_iprev + in * P.nL, *vdprev = R.D_vdprev + in * P.nD;
  int32_t *ison = R.S_ison + in * P.nS;
  const double dtc = spicey_exact_max(R.dt, SPICEY_EPS);
  const int n_el = P.nR + P.nC + P.nL + P.nS + P.nV + P.nD;
  // scal: [0, 1] active rows of the pivot step (by parity: a counter is cleared two steps after it was read), [2] skipped
  // multipliers of the solve, [4, 5] switched (by iteration parity)
  auto volt = [&](int node) { return node == 0 ? 0.0 : x[node - 1]; };
  int64_t skipped = 0, solves = 0;
  int code = 0, err_iter = 0;
  int64_t step = 0;
  ex.phase(SPICEY_PH_PRO, [&](int tid) {
    if (tid == 0) { scal[4] = 0; scal[5] = 0; }
  });
  for (; step <= R.steps && code == 0; step++) {
    const double *src = R.src + in * R.src_stride + (size_t)step * P.nV;
    int iter = 0;
    for (; iter < SPICEY_MAX_ITER; iter++) {
      // ---- the iteration's quantities (one thread per element; diodes linearised at vdPrev or the last iterate), a zero
      //      A | b and the identity row order
      ex.phase(SPICEY_PH_B, [&](int tid) {
        for (int e = tid; e < n_el; e += T) {
          int i = e;
          if (i < P.nR) { q[P.qR + i] = 1 / Rv[i]; continue; }
          i -= P.nR;
          if (i < P.nC) {
            const double Gc = Cv[i] / dtc;
            q[P.qGc + i] = Gc;
            q[P.qIc + i] = -Gc * vprev[i];
            continue;
          }
          i -= P.nC;
          if (i < P.nL) { q[P.qGl + i] = dtc / Lv[i]; q[P.qIl + i] = iprev[i]; continue; }
          i -= P.nL;
          if (i < P.nS) {
            const double Rvalue = ison[i] ? Ron[i] : Roff[i];
            q[P.qS + i] = 1 / spicey_exact_max(fabs(Rvalue), SPICEY_EPS);
            continue;
          }
          i -= P.nS;
          if (i < P.nV) { q[P.qV + i] = src[i]; continue; }
          i -= P.nV;
          const double vd_iter = volt(P.D_nd[2 * i]) - volt(P.D_nd[2 * i + 1]);
          const double vd = iter == 0 ? vdprev[i] : vd_iter;
          vdlin[i] = vd;
          const double vt = Dn[i] * SPICEY_VT300;
          double vl = vd;
          if (vd > 0.8) vl = 0.8;
          if (vd < -1.0) vl = -1.0;
          const double ee = spicey_fdlibm_exp(vl / vt);
          const double id = Dis[i] * (ee - 1);
          const double gd = spicey_exact_max((Dis[i] / vt) * ee, 1e-12);
          q[P.qGd + i] = gd;
          q[P.qIeq + i] = id - gd * vl;
        }
        if (tid == 0) { q[P.qOne] = 1.0; scal[0] = 0; scal[1] = 0; scal[2] = 0; }
        for (size_t i = (size_t)tid; i < (size_t)n * (size_t)ld; i += (size_t)T) A[i] = 0.0;
        for (int i = tid; i < n; i += T) perm[i] = i;
      });
      // ---- stamps: every entry sums its contributions in the reference's order
      ex.phase(SPICEY_PH_B, [&](int tid) {
        if (tid == 0) scal[4 + ((iter + 1) & 1)] = 0;  // (the next iteration's switch counter, last read before the phase above)
        for (int e = tid; e < P.nEnt; e += T) {
          double s = 0.0;
          for (uint32_t c = P.ent_ptr[e]; c < P.ent_ptr[e + 1]; c++) {
            const uint32_t w = P.ent_src[c];
            const double v = q[w & ~SPICEY_EXACT_SUB];
            s = (w & SPICEY_EXACT_SUB) ? s - v : s + v;
          }
          A[P.ent_pos[e]] = s;
        }
      });
      // ---- forward elimination (solveReal.ts:15-53)
      bool singular = false;
      for (int k = 0; k < n; k++) {
        double bv;
        int bi;
        ex.argmax(n - k, [&](int j) { return fabs(A[(size_t)perm[k + j] * ld + k]); }, bv, bi);
        const double akk = fabs(A[(size_t)perm[k] * ld + k]);
        if (akk != akk) { bv = akk; bi = 0; }  // (a NaN on the diagonal: no |a_ik| > NaN, the reference keeps row k)
        if (bv < SPICEY_EPS) { singular = true; break; }
        const int imax = k + bi;
        const int pr = perm[imax], kr = perm[k];
        const double *prow = A + (size_t)pr * ld;
        const double pivot = prow[k];
        int32_t *na_k = scal + (k & 1);
        ex.phase(SPICEY_PH_U0, [&](int tid) {
          if (tid == 0) scal[(k + 1) & 1] = 0;
          for (int i = k + 1 + tid; i < n; i += T) {
            const int r = i == imax ? kr : perm[i];
            const double f = A[(size_t)r * ld + k] / pivot;
            if (fabs(f) < SPICEY_EPS) {  // solveReal.ts:46
              if (f != 0.0) ex.atomic_add(&scal[2], 1);
              continue;
            }
            const int a = ex.atomic_add(na_k, 1);
            act_r[a] = r;
            act_f[a] = f;
          }
          // nonzero columns j > k of the pivot row (its values are final now): the back substitution visits only those
          for (int w = ((k + 1) >> 5) + tid; w < mw; w += T) {
            uint32_t bits = 0;
            for (int b = 0; b < 32; b++) {
              const int j = w * 32 + b;
              if (j > k && j < n && prow[j] != 0.0) bits |= 1u << b;
            }
            mask[(size_t)k * mw + w] = bits;
          }
        });
        const int na = *na_k;
        // the row swap (after every thread has read pr, kr) and row[j] = row[j] - f * prow[j], j = k + 1 .. n (column k of
        // the rows below is never read again); a wave per row
        if (na > 0 || imax != k)
          ex.phase(SPICEY_PH_U0, [&](int tid) {
            if (tid == 0) {
              perm[k] = pr;
              perm[imax] = kr;
            }
            const int nw = (T + 63) >> 6, wv = tid >> 6, lane = tid & 63;
            for (int a = wv; a < na; a += nw) {
              double *row = A + (size_t)act_r[a] * ld;
              const double f = act_f[a];
              for (int j = k + 1 + lane; j <= n; j += 64) row[j] = row[j] - f * prow[j];
            }
          });
      }
      if (singular) { code = SPICEY_ERR_SINGULAR; err_iter = iter; break; }
      skipped += scal[2];
      solves++;
      // ---- back substitution (solveReal.ts:56-72): s = b_i; s -= a_ij * x_j for j = i+1 .. n-1 ascending; x_i = s / a_ii.
      //      A term with a_ij = +-0 changes s only when s = -0 or x_j is not finite: such terms are taken in order exactly
      //      then, and skipped otherwise (mask = the nonzero columns of the row).
      ex.phase(SPICEY_PH_K0, [&](int tid) {
        if (tid != 0) return;
        bool all_terms = false;  // an x_j that is not finite: from here on every term is taken
        for (int i = n - 1; i >= 0; i--) {
          const double *row = A + (size_t)perm[i] * ld;
          double s = row[n];
          if (all_terms) {
            for (int j = i + 1; j < n; j++) s -= row[j] * x[j];
          } else {
            int jn = i + 1;  // first column not taken yet
            for (int w = (i + 1) >> 5; w < mw; w++) {
              uint32_t bits = mask[(size_t)i * mw + w];
              while (bits) {
                const int j = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                if (j <= i) continue;
                if (spicey_exact_is_neg_zero(s))
                  for (int jj = jn; jj < j; jj++) s -= row[jj] * x[jj];
                s -= row[j] * x[j];
                jn = j + 1;
              }
            }
            if (spicey_exact_is_neg_zero(s))
              for (int jj = jn; jj < n; jj++) s -= row[jj] * x[jj];
          }
          const double xi = s / row[i];
          x[i] = xi;
          if (!isfinite(xi)) all_terms = true;
        }
      });
      // ---- switches (simulateTRAN.ts:108-128)
      if (P.nS == 0) break;
      int32_t *sw = scal + 4 + (iter & 1);
      ex.phase(SPICEY_PH_S, [&](int tid) {
        for (int i = tid; i < P.nS; i += T) {
          const double vctrl = volt(P.S_ctl[2 * i]) - volt(P.S_ctl[2 * i + 1]);
          int next = ison[i];
          if (ison[i]) {
            if (vctrl < Voff[i]) next = 0;
          } else if (vctrl > Von[i]) {
            next = 1;
          }
          if (next != ison[i]) {
            ison[i] = next;
            ex.atomic_add(sw, 1);
          }
        }
      });
      if (*sw == 0) break;
      if (iter == SPICEY_MAX_ITER - 1) break;
    }
    if (code != 0) break;
    // ---- recording (simulateTRAN.ts:164-219) and the diagnostics
    const int64_t np = R.steps + 1;
    ex.phase(SPICEY_PH_Z, [&](int tid) {
      if (tid == 0) {
        if (R.iters) R.iters[in * np + step] = iter + 1;
        if (R.lin_err) {
          double m = 0.0;
          for (int i = 0; i < P.nD; i++) {
            const double e = fabs((volt(P.D_nd[2 * i]) - volt(P.D_nd[2 * i + 1])) - vdlin[i]);
            if (e > m) m = e;
          }
          uint64_t b;
          __builtin_memcpy(&b, &m, 8);
          R.lin_err[in * np + step] = (unsigned long long)b;
        }
      }
      double *ov = R.out_v + (in * np + step) * P.nOut;
      for (int i = tid; i < P.nOut; i += T) ov[i] = volt(P.out_nodes[i]);
      if (!R.out_i) return;
      double *oi = R.out_i + (in * np + step) * P.nCur;
      for (int e = tid; e < n_el; e += T) {
        int i = e;
        if (i < P.nR) { oi[e] = (volt(P.R_nd[2 * i]) - volt(P.R_nd[2 * i + 1])) / Rv[i]; continue; }
        i -= P.nR;
        if (i < P.nC) { oi[e] = (Cv[i] * (volt(P.C_nd[2 * i]) - volt(P.C_nd[2 * i + 1]) - vprev[i])) / dtc; continue; }
        i -= P.nC;
        if (i < P.nL) { oi[e] = (dtc / Lv[i]) * (volt(P.L_nd[2 * i]) - volt(P.L_nd[2 * i + 1])) + iprev[i]; continue; }
        i -= P.nL;
        // (recording order R, C, L, V, S, D)
        if (i < P.nV) { oi[P.nR + P.nC + P.nL + i] = x[P.nN + i]; continue; }
        i -= P.nV;
        if (i < P.nS) {
          const double Rvalue = ison[i] ? Ron[i] : Roff[i];
          oi[P.nR + P.nC + P.nL + P.nV + i] = (volt(P.S_nd[2 * i]) - volt(P.S_nd[2 * i + 1])) / spicey_exact_max(fabs(Rvalue), SPICEY_EPS);
          continue;
        }
        i -= P.nS;
        const double vd = volt(P.D_nd[2 * i]) - volt(P.D_nd[2 * i + 1]);
        const double vt = Dn[i] * SPICEY_VT300;
        oi[e] = Dis[i] * (spicey_fdlibm_exp(vd / vt) - 1);
      }
    });
    // ---- state update (simulateTRAN.ts:221-237)
    ex.phase(SPICEY_PH_Z, [&](int tid) {
      for (int i = tid; i < P.nC; i += T) vprev[i] = volt(P.C_nd[2 * i]) - volt(P.C_nd[2 * i + 1]);
      for (int i = tid; i < P.nL; i += T) iprev[i] = (dtc / Lv[i]) * (volt(P.L_nd[2 * i]) - volt(P.L_nd[2 * i + 1])) + iprev[i];
      for (int i = tid; i < P.nD; i += T) vdprev[i] = volt(P.D_nd[2 * i]) - volt(P.D_nd[2 * i + 1]);
    });
  }
  ex.phase(SPICEY_PH_Z, [&](int tid) {
    if (tid != 0) return;
    R.status[(size_t)wg * 4 + 0] = code;
    R.status[(size_t)wg * 4 + 1] = code ? inst : 0;
    R.status[(size_t)wg * 4 + 2] = code ? (int32_t)step : 0;
    R.status[(size_t)wg * 4 + 3] = code ? err_iter : 0;
    R.solves[wg] = (unsigned long long)solves;
    if (R.skip_risk) R.skip_risk[in] = (unsigned long long)skipped;
  });
}
