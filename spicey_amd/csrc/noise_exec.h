// noise_exec.h — thermal noise out of an injected AC sweep: the one definition of the reduction, used by the kernels of
// noise.hip and by the CPU harness of tests/noise_host (compiled without FMA contraction on both sides, so the two give the
// same bits).
//
// The sweep (ac_exec.h, SpiceyAcRun::inj_*) solved A x = e_p - e_n with every source phasor at zero.  A is complex
// symmetric, so x is the adjoint solution (DESIGN.md "Noise analysis"): with out = v(p) - v(n),
//   x[p] - x[n]          = Z_out
//   i(V_in)              = the voltage gain V_in -> out
//   i(R_k) = (x_a - x_b) / R_k = the gain to out of a voltage source in series with R_k
// and the output noise density is the sum over the resistors of 4kT R_k |i(R_k)|^2.  Inputs: d_i [n_inst][n_freq][n_cur][2]
// whose first nR columns are the resistors' currents, d_v [n_inst][n_freq][n_v][2], R [n_inst][nR] in ohms, freqs [n_freq].
//
// Operation order (every operation rounded on its own):
//   sample      p = re re + im im;  c = (kt4 R) p
//   spectrum    one wave per (instance, frequency): lane l adds c of the resistors r = l, l + 64, ... in ascending r to
//               +0.0; the 64 partials meet by s[l] += s[l + stride] for stride = 32, 16, ..., 1; lane 0 holds onoise.
//               d_spec [n_inst][n_freq][4] = {onoise, gain2 = |i(V_in)|^2 or 0, zout_re, zout_im}, zout = v(out_p) - v(out_n)
//               with one rounded subtraction per part (a column of -1 is ground: nothing is subtracted or 0 is read).
//   band        one thread per (instance, row), rows 0 .. nR + 1, trapezoidal rule over the window [k0, k1] in ascending k:
//               acc = +0.0;  acc += (0.5 (y_k + y_k+1)) (f_k+1 - f_k)
//               row r < nR: y = c of resistor r -> d_contrib [n_inst][nR]; row nR: y = onoise -> d_total[inst][0]; row
//               nR + 1: y = onoise / gain2, the IEEE quotient (inf and NaN are left to show) -> d_total[inst][1].
// Nothing is square-rooted, logged or compared in floating point: RMS values, decibels, rankings and inoise per frequency
// are the host's.  A result is a function of the window's samples and the request alone.
#pragma once
#include <stdint.h>

#include "measure_exec.h"

#define SPICEY_NOISE_LANES 64     // one (instance, frequency) per wave
#define SPICEY_NOISE_THREADS 256  // workgroup size of both kernels
#define SPICEY_NOISE_SPEC 4       // doubles of a spectrum row

// A validated request with the buffers it runs on, as the kernels read it (noise.h: spicey_noise_judge).
struct SpiceyNoiseArgs {
  const double *d_i, *d_v, *R, *freqs;
  double kt4;
  int64_t n_freq, k0, k1;
  int32_t n_inst, nR, n_cur, n_v;
  int32_t out_p, out_n, in_col, pad_;
};

SPICEY_MEAS_HD double spicey_noise_sample(double kt4, double R, double re, double im) {
  const double p = re * re + im * im;
  return (kt4 * R) * p;
}

// c of resistor r at (inst, k)
SPICEY_MEAS_HD double spicey_noise_c(const SpiceyNoiseArgs &A, int64_t inst, int64_t k, int32_t r) {
  const double *s = A.d_i + ((inst * A.n_freq + k) * A.n_cur + r) * 2;
  return spicey_noise_sample(A.kt4, A.R[inst * A.nR + r], s[0], s[1]);
}

// Lane `lane` of the wave of slot = inst * n_freq + k: its partial of onoise.  Lane l reads the 16 bytes behind lane l - 1's.
SPICEY_MEAS_HD double spicey_noise_lane(const SpiceyNoiseArgs &A, int64_t slot, int32_t lane) {
  const int64_t inst = slot / A.n_freq;
  const double *row = A.d_i + slot * A.n_cur * 2;
  const double *Rv = A.R + inst * A.nR;
  double s = 0.0;
  for (int32_t r = lane; r < A.nR; r += SPICEY_NOISE_LANES) s = s + spicey_noise_sample(A.kt4, Rv[r], row[2 * r], row[2 * r + 1]);
  return s;
}

// What lane 0 writes once the partials have met.
SPICEY_MEAS_HD void spicey_noise_spec_row(const SpiceyNoiseArgs &A, int64_t slot, double onoise, double *spec) {
  double *dst = spec + slot * SPICEY_NOISE_SPEC;
  double g2 = 0.0;
  if (A.in_col >= 0) {
    const double *s = A.d_i + (slot * A.n_cur + A.in_col) * 2;
    g2 = s[0] * s[0] + s[1] * s[1];
  }
  const double *v = A.d_v + slot * A.n_v * 2;
  double zr = 0.0, zi = 0.0;
  if (A.out_p >= 0) { zr = v[2 * A.out_p]; zi = v[2 * A.out_p + 1]; }
  if (A.out_n >= 0) { zr = zr - v[2 * A.out_n]; zi = zi - v[2 * A.out_n + 1]; }
  dst[0] = onoise; dst[1] = g2; dst[2] = zr; dst[3] = zi;
}

// The band kernel's thread idx = inst * (nR + 2) + row: neighbouring threads read neighbouring resistors of one row of d_i.
SPICEY_MEAS_HD void spicey_noise_band(const SpiceyNoiseArgs &A, int64_t idx, const double *spec, double *contrib, double *total) {
  const int64_t rows = (int64_t)A.nR + 2;
  const int64_t inst = idx / rows;
  const int32_t row = (int32_t)(idx - inst * rows);
  const double *sp = spec + inst * A.n_freq * SPICEY_NOISE_SPEC;
  double acc = 0.0;
  if (row < A.nR) {
    double y0 = spicey_noise_c(A, inst, A.k0, row);
    for (int64_t k = A.k0; k < A.k1; k++) {
      const double y1 = spicey_noise_c(A, inst, k + 1, row);
      acc = acc + (0.5 * (y0 + y1)) * (A.freqs[k + 1] - A.freqs[k]);
      y0 = y1;
    }
    contrib[inst * A.nR + row] = acc;
  } else if (row == A.nR) {
    for (int64_t k = A.k0; k < A.k1; k++)
      acc = acc + (0.5 * (sp[k * SPICEY_NOISE_SPEC] + sp[(k + 1) * SPICEY_NOISE_SPEC])) * (A.freqs[k + 1] - A.freqs[k]);
    total[inst * 2] = acc;
  } else {
    double y0 = sp[A.k0 * SPICEY_NOISE_SPEC] / sp[A.k0 * SPICEY_NOISE_SPEC + 1];
    for (int64_t k = A.k0; k < A.k1; k++) {
      const double y1 = sp[(k + 1) * SPICEY_NOISE_SPEC] / sp[(k + 1) * SPICEY_NOISE_SPEC + 1];
      acc = acc + (0.5 * (y0 + y1)) * (A.freqs[k + 1] - A.freqs[k]);
      y0 = y1;
    }
    total[inst * 2 + 1] = acc;
  }
}
