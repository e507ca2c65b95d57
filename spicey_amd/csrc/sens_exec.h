// sens_exec.h — first-order AC sensitivities out of a direct and an adjoint sweep: the one definition of the reduction, used by
// the kernels of sens.hip and by the CPU harness of tests/sens_host (compiled without FMA contraction on both sides, so the
// two give the same bits).
//
// Sweep D (plain, the netlist's phasors) and sweep X (every phasor zero, a unit current injected into the output pair) both
// recorded the element currents i = Y dv (ac_exec.h).  The AC matrix of R, C, L and V is complex symmetric, so X is the adjoint
// solution and, with out = v(p) - v(n), d out / d Y_e = - dx_e dd_e (DESIGN.md "AC sensitivities").  Inputs: d_id, d_ix
// [n_inst][n_freq][n_cur][2] whose first nR + nC + nL columns are the elements' currents (R, then C, then L), d_v
// [n_inst][n_freq][n_v][2] of sweep D, R / C / L [n_inst][n<kind>] in ohms, farads and henries, tol [nE], freqs [n_freq].
//
// Operation order (every operation rounded on its own), x = i_X(e), y = i_D(e), p the element's value:
//   product     pr = x.re y.re - x.im y.im;  pi = x.re y.im + x.im y.re
//   absolute    R: S = (p pr, p pi)
//               C: q = w p with w = (2 pi) f as the engine forms it; S = (-pi / q, pr / q), or (+0.0, +0.0) where q == 0
//               L: q = w p; S = (-pi q, pr q)
//   output      H = v(out_p) - v(out_n) of sweep D, one rounded subtraction per part (a column of -1 is ground: nothing is
//               subtracted or 0 is read); d = H.re H.re + H.im H.im
//   relative    m = (S.re H.re + S.im H.im) / d;  phi = (S.im H.re - S.re H.im) / d    (IEEE quotients: d == 0 shows inf / NaN)
//   spectrum    one wave per (instance, frequency): lane l adds, over the elements e = l, l + 64, ... in ascending e and from
//               +0.0, the four sums t |m|, (t m)(t m), t |phi|, (t phi)(t phi) with t = tol[e]; the 64 partials of each meet by
//               s[l] += s[l + stride] for stride = 32, 16, ..., 1; lane 0 writes
//               d_spec [n_inst][n_freq][6] = {H.re, H.im, wc_mag, var_mag, wc_ph, var_ph}.
//               With d_full, every lane also writes {m, phi} of its elements to d_full [n_inst][n_freq][nE][2].
//   peak        one thread per (instance, element) walks the window [k0, k1] in ascending k recomputing m and phi; it starts
//               with the value at k0 and replaces it where fabs(new) > fabs(best) (the first of equal magnitudes stays, a NaN
//               at k0 stays); d_peak [n_inst][nE][4] = {m at its peak, its k, phi at its peak, its k}, indices as doubles.
// Nothing is square-rooted or logged: sigmas, decibels, degrees and rankings are the host's.  A result is a function of the
// samples and the request alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "measure_exec.h"

#define SPICEY_SENS_LANES 64     // one (instance, frequency) per wave
#define SPICEY_SENS_THREADS 256  // workgroup size of both kernels
#define SPICEY_SENS_SPEC 6       // doubles of a spectrum row
#define SPICEY_SENS_PEAK 4       // doubles of a peak row

// A validated request with the buffers it runs on, as the kernels read it (sens.h: spicey_sens_judge).
struct SpiceySensArgs {
  const double *d_v, *d_id, *d_ix, *R, *C, *L, *tol, *freqs;
  int64_t n_freq, k0, k1;
  int32_t n_inst, nR, nC, nL, n_cur, n_v, out_p, out_n;
};

struct SpiceySensH { double re, im, d; };

// H and |H|^2 of slot = inst * n_freq + k
SPICEY_MEAS_HD SpiceySensH spicey_sens_h(const SpiceySensArgs &A, int64_t slot) {
  const double *v = A.d_v + slot * A.n_v * 2;
  SpiceySensH h{0.0, 0.0, 0.0};
  if (A.out_p >= 0) { h.re = v[2 * A.out_p]; h.im = v[2 * A.out_p + 1]; }
  if (A.out_n >= 0) { h.re = h.re - v[2 * A.out_n]; h.im = h.im - v[2 * A.out_n + 1]; }
  h.d = h.re * h.re + h.im * h.im;
  return h;
}

// w of frequency index k, the engine's product (ac_exec.h)
SPICEY_MEAS_HD double spicey_sens_w(const SpiceySensArgs &A, int64_t k) {
  const double two_pi = 2 * 3.141592653589793;
  return two_pi * A.freqs[k];
}

// {m, phi} of element e at (inst, slot): the whole arithmetic of one (frequency, element)
SPICEY_MEAS_HD void spicey_sens_rel(const SpiceySensArgs &A, int64_t inst, int64_t slot, int32_t e, double w, const SpiceySensH &h, double *m, double *phi) {
  const double *x = A.d_ix + (slot * A.n_cur + e) * 2, *y = A.d_id + (slot * A.n_cur + e) * 2;
  const double xr = x[0], xi = x[1], yr = y[0], yi = y[1];
  const double pr = xr * yr - xi * yi;
  const double pi = xr * yi + xi * yr;
  double sr, si;
  if (e < A.nR) {
    const double s = A.R[inst * A.nR + e];
    sr = s * pr; si = s * pi;
  } else if (e < A.nR + A.nC) {
    const double q = w * A.C[inst * A.nC + (e - A.nR)];
    if (q == 0.0) { sr = 0.0; si = 0.0; }
    else { sr = -pi / q; si = pr / q; }
  } else {
    const double q = w * A.L[inst * A.nL + (e - A.nR - A.nC)];
    sr = -pi * q; si = pr * q;
  }
  *m = (sr * h.re + si * h.im) / h.d;
  *phi = (si * h.re - sr * h.im) / h.d;
}

// Lane `lane` of the wave of slot = inst * n_freq + k: its partials s[4].  Lane l reads the 16 bytes behind lane l - 1's.
SPICEY_MEAS_HD void spicey_sens_lane(const SpiceySensArgs &A, int64_t slot, int32_t lane, double *full, double *s) {
  const int64_t inst = slot / A.n_freq;
  const int32_t nE = A.nR + A.nC + A.nL;
  const SpiceySensH h = spicey_sens_h(A, slot);
  const double w = spicey_sens_w(A, slot - inst * A.n_freq);
  double *frow = full ? full + slot * nE * 2 : nullptr;
  s[0] = 0.0; s[1] = 0.0; s[2] = 0.0; s[3] = 0.0;
  for (int32_t e = lane; e < nE; e += SPICEY_SENS_LANES) {
    double m, phi;
    spicey_sens_rel(A, inst, slot, e, w, h, &m, &phi);
    const double t = A.tol[e];
    const double tm = t * m, tp = t * phi;
    s[0] = s[0] + t * fabs(m);
    s[1] = s[1] + tm * tm;
    s[2] = s[2] + t * fabs(phi);
    s[3] = s[3] + tp * tp;
    if (frow) { frow[2 * e] = m; frow[2 * e + 1] = phi; }
  }
}

// What lane 0 writes once the partials have met.
SPICEY_MEAS_HD void spicey_sens_spec_row(const SpiceySensArgs &A, int64_t slot, const double *s, double *spec) {
  const SpiceySensH h = spicey_sens_h(A, slot);
  double *dst = spec + slot * SPICEY_SENS_SPEC;
  dst[0] = h.re; dst[1] = h.im; dst[2] = s[0]; dst[3] = s[1]; dst[4] = s[2]; dst[5] = s[3];
}

// The peak kernel's thread idx = inst * nE + e: neighbouring threads read neighbouring elements of one k.
SPICEY_MEAS_HD void spicey_sens_peak(const SpiceySensArgs &A, int64_t idx, double *peak) {
  const int64_t nE = (int64_t)A.nR + A.nC + A.nL;
  const int64_t inst = idx / nE;
  const int32_t e = (int32_t)(idx - inst * nE);
  double bm = 0.0, bp = 0.0;
  int64_t km = A.k0, kp = A.k0;
  for (int64_t k = A.k0; k <= A.k1; k++) {
    const int64_t slot = inst * A.n_freq + k;
    const SpiceySensH h = spicey_sens_h(A, slot);
    double m, phi;
    spicey_sens_rel(A, inst, slot, e, spicey_sens_w(A, k), h, &m, &phi);
    if (k == A.k0) { bm = m; bp = phi; continue; }
    if (fabs(m) > fabs(bm)) { bm = m; km = k; }
    if (fabs(phi) > fabs(bp)) { bp = phi; kp = k; }
  }
  double *dst = peak + idx * SPICEY_SENS_PEAK;
  dst[0] = bm; dst[1] = (double)km; dst[2] = bp; dst[3] = (double)kp;
}
