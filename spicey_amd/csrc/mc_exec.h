// mc_exec.h — Monte Carlo tolerance analysis of the AC sweep: the one definition of the draw and of the reduction across
// instances, used by the kernels of mc.hip and by the CPU harness of tests/mc_host (compiled without FMA contraction on both
// sides, so the two give the same bits).
//
// The draw.  One thread per (sample s, element e), e in the column order of out_i: the nR resistors, the nC capacitors, the nL
// inductors.  Integer arithmetic up to the last three floating-point operations:
//   random bits  Philox4x32-10, counter (s, e, 0, 0), key (seed & 0xffffffff, seed >> 32): multipliers 0xD2511F53 on c0 and
//                0xCD9E8D57 on c2, one round (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
//                the Weyl constants 0x9E3779B9 / 0xBB67AE85 added to the key after each round
//   uniform      m = (x0 << 20) | (x1 >> 12), 52 bits
//   deviate      a table icdf[K + 1], K = 2^L, built by the host (no transcendental here): j = m >> (52 - L), r the low 52 - L
//                bits, frac = (double)r 2^-(52 - L) (exact), d = icdf[j] + frac (icdf[j + 1] - icdf[j]) — one rounded subtraction,
//                one product, one addition
//   scaling      g = 1 + tol[e] d;  C and L become nom g;  R' = R g in ohms and the sweep's array gets the IEEE quotient 1.0 / R'
//   keep_first   sample 0 takes g = 1 without drawing: its rows are the nominal bits (1.0 / (R 1.0) = 1.0 / R)
// The nominal values are rows of their own per sample, [n_inst][n<kind>], as an AC handle holds them.
//
// The reduction.  q[s][k] = H.re H.re + H.im H.im of H = v(out_p) - v(out_n) (one rounded subtraction per part, a column of -1 is
// ground, as sens_exec.h).  q >= +0 or NaN, so bits(q) & 0x7fff...ffff — the key — orders the values as unsigned integers: NaNs
// behind +inf, and 0xffff...ffff (invalid samples, the padding up to n_pad = the next power of two >= n_inst) last.
//   per sample     one wave per s < n_pad, lanes striding k: the key into qT[k][s]; with a mask the violations
//                  !(q >= lo[k] && q <= hi[k]) (a NaN violates) counted and the lowest violating k kept, integers that meet
//                  across the lanes; d_sample [n_inst][2] = {count, lowest k or -1}, {-1, -1} for an invalid sample
//   per frequency  one workgroup per k: row k of qT into LDS, a bitonic network on the unsigned keys (spicey_mc_sort), then wave 0:
//                  lane l adds x[l], x[l + 64], ... of the first n_valid sorted values in ascending index to +0.0, once as they
//                  are and once squared, and counts their violations of the mask at k; the 64 partials meet by
//                  s[l] += s[l + stride], stride 32 .. 1;  d_freq [n_freq][4 + n_rank] = {n_valid, violating samples, sum q,
//                  sum q q, the sorted values at the n_rank ranks}
// Apart from the two sums nothing is a floating-point accumulation, and no floating-point comparison orders anything: a
// result is a function of the samples and the request alone, not of the geometry.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "measure_exec.h"

#define SPICEY_MC_LANES 64         // one sample per wave (per-sample kernel); the summing wave of the per-frequency kernel
#define SPICEY_MC_THREADS 256      // workgroup size of the draw and of the per-sample kernel
#define SPICEY_MC_SORT_MAX 1024    // most threads of a sorting workgroup
#define SPICEY_MC_MAX_LOG2K 12     // the table has at most 4096 intervals
#define SPICEY_MC_MAX_INST 16384   // n_pad 8-byte keys in LDS: 128 KiB
#define SPICEY_MC_FREQ_HEAD 4      // doubles of a d_freq row before the order statistics
#define SPICEY_MC_PAD_KEY 0xffffffffffffffffull

// A validated draw with the buffers it runs on, as the kernel reads it (mc.h: spicey_mc_draw_judge).
struct SpiceyMcDrawArgs {
  const double *R, *C, *L;  // nominal [n_inst][n<kind>]: ohms, farads, henries
  const double *tol, *icdf; // [nE], [K + 1] (the launcher points them into the workspace)
  double *oR, *oC, *oL;     // drawn [n_inst][n<kind>]: 1 / ohms, farads, henries
  uint64_t seed;
  int32_t n_inst, nR, nC, nL, log2K, keep_first;
};

// A validated reduction with the buffers it runs on (mc.h: spicey_mc_reduce_judge).  valid, lo, hi, ranks and qT lie in the
// workspace; valid is null when every sample is valid, lo is null without a mask (then hi is too).
struct SpiceyMcReduceArgs {
  const double *d_v;        // [n_inst][n_freq][n_v][2]
  const uint8_t *valid;     // [n_inst]
  const double *lo, *hi;    // [n_freq] limits of |H|^2
  const int64_t *ranks;     // [n_rank], each in [0, n_valid)
  uint64_t *qT;             // [n_freq][n_pad]
  int64_t n_freq;
  int32_t n_inst, n_pad, n_valid, n_v, out_p, out_n, n_rank, sort_threads;
};

SPICEY_MEAS_HD uint64_t spicey_mc_bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof(u));
  return u;
}
SPICEY_MEAS_HD double spicey_mc_double(uint64_t u) {
  double x;
  memcpy(&x, &u, sizeof(x));
  return x;
}

// Philox4x32-10 in place: c the counter, k0 / k1 the key.
SPICEY_MEAS_HD void spicey_mc_philox(uint32_t *c, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the 52 uniform bits of (sample s, element e)
SPICEY_MEAS_HD uint64_t spicey_mc_uniform(uint64_t seed, uint32_t s, uint32_t e) {
  uint32_t c[4] = {s, e, 0u, 0u};
  spicey_mc_philox(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  return ((uint64_t)c[0] << 20) | (uint64_t)(c[1] >> 12);
}

// the deviate of m in units of the tolerance: the table interpolated at m 2^-52
SPICEY_MEAS_HD double spicey_mc_deviate(const double *icdf, int32_t log2K, uint64_t m) {
  const int32_t sh = 52 - log2K;
  const uint64_t j = m >> sh, r = m & (((uint64_t)1 << sh) - 1);
  const double scale = spicey_mc_double((uint64_t)(1023 - sh) << 52);  // 2^-sh
  const double frac = (double)r * scale;
  const double a = icdf[j], step = icdf[j + 1] - a;
  return a + frac * step;
}

// Thread idx = s * nE + e of the draw.
SPICEY_MEAS_HD void spicey_mc_draw(const SpiceyMcDrawArgs &A, int64_t idx) {
  const int64_t nE = (int64_t)A.nR + A.nC + A.nL;
  const int64_t s = idx / nE;
  const int32_t e = (int32_t)(idx - s * nE);
  double g = 1.0;
  if (!(A.keep_first && s == 0)) {
    const double d = spicey_mc_deviate(A.icdf, A.log2K, spicey_mc_uniform(A.seed, (uint32_t)s, (uint32_t)e));
    g = 1.0 + A.tol[e] * d;
  }
  if (e < A.nR) {
    const int64_t at = s * A.nR + e;
    const double r = A.R[at] * g;
    A.oR[at] = 1.0 / r;
  } else if (e < A.nR + A.nC) {
    const int64_t at = s * A.nC + (e - A.nR);
    A.oC[at] = A.C[at] * g;
  } else {
    const int64_t at = s * A.nL + (e - A.nR - A.nC);
    A.oL[at] = A.L[at] * g;
  }
}

// |H|^2 of slot = s * n_freq + k
SPICEY_MEAS_HD double spicey_mc_q(const SpiceyMcReduceArgs &A, int64_t slot) {
  const double *v = A.d_v + slot * A.n_v * 2;
  double re = 0.0, im = 0.0;
  if (A.out_p >= 0) { re = v[2 * A.out_p]; im = v[2 * A.out_p + 1]; }
  if (A.out_n >= 0) { re = re - v[2 * A.out_n]; im = im - v[2 * A.out_n + 1]; }
  return re * re + im * im;
}

SPICEY_MEAS_HD bool spicey_mc_violates(const SpiceyMcReduceArgs &A, int64_t k, double q) { return A.lo && !(q >= A.lo[k] && q <= A.hi[k]); }

// Lane `lane` of the wave of sample s < n_pad: writes its keys of column s of qT, returns its violations and its lowest
// violating k (-1: none).
SPICEY_MEAS_HD void spicey_mc_sample_lane(const SpiceyMcReduceArgs &A, int64_t s, int32_t lane, int64_t *count, int64_t *first) {
  const bool ok = s < A.n_inst && (!A.valid || A.valid[s]);
  int64_t n = 0, f = -1;
  for (int64_t k = lane; k < A.n_freq; k += SPICEY_MC_LANES) {
    uint64_t key = SPICEY_MC_PAD_KEY;
    if (ok) {
      const double q = spicey_mc_q(A, s * A.n_freq + k);
      key = spicey_mc_bits(q) & 0x7fffffffffffffffull;
      if (spicey_mc_violates(A, k, q)) {
        n++;
        if (f < 0) f = k;
      }
    }
    A.qT[k * A.n_pad + s] = key;
  }
  *count = n;
  *first = f;
}

// How two lanes' {count, first} meet (integers: any order gives the same).
SPICEY_MEAS_HD void spicey_mc_sample_meet(int64_t *count, int64_t *first, int64_t c2, int64_t f2) {
  *count += c2;
  if (f2 >= 0 && (*first < 0 || f2 < *first)) *first = f2;
}

// What lane 0 writes once the lanes have met.
SPICEY_MEAS_HD void spicey_mc_sample_row(const SpiceyMcReduceArgs &A, int64_t s, int64_t count, int64_t first, int64_t *sample) {
  if (s >= A.n_inst) return;
  const bool ok = !A.valid || A.valid[s];
  sample[2 * s] = ok ? count : -1;
  sample[2 * s + 1] = ok ? first : -1;
}

// The n_pad keys of x in ascending unsigned order by a workgroup of `threads` threads.  par(f) runs f(t) for every thread t of
// the workgroup and ends with a barrier: the kernel's is { f(threadIdx.x); __syncthreads(); }, the harness's a loop over t.  A
// stage's n_pad / 2 pairs are disjoint, so who takes which does not matter.
template <class Par>
SPICEY_MEAS_HD void spicey_mc_sort(Par par, int32_t threads, uint64_t *x, int32_t n_pad) {
  const int32_t half = n_pad >> 1;
  for (int32_t size = 2; size <= n_pad; size <<= 1)
    for (int32_t stride = size >> 1; stride > 0; stride >>= 1)
      par([&](int32_t t) {
        for (int32_t p = t; p < half; p += threads) {
          const int32_t i = 2 * p - (p & (stride - 1)), j = i + stride;
          const bool up = (i & size) == 0 || size == n_pad;
          const uint64_t a = x[i], b = x[j];
          if ((a > b) == up && a != b) { x[i] = b; x[j] = a; }
        }
      });
}

// Lane `lane` of the summing wave over the sorted keys x of frequency k: s[0] = its sum of q, s[1] of q q, *viol its count.
SPICEY_MEAS_HD void spicey_mc_freq_lane(const SpiceyMcReduceArgs &A, int64_t k, const uint64_t *x, int32_t lane, double *s, int64_t *viol) {
  s[0] = 0.0; s[1] = 0.0;
  int64_t n = 0;
  for (int32_t i = lane; i < A.n_valid; i += SPICEY_MC_LANES) {
    const double q = spicey_mc_double(x[i]);
    s[0] = s[0] + q;
    s[1] = s[1] + q * q;
    n += spicey_mc_violates(A, k, q) ? 1 : 0;
  }
  *viol = n;
}

// What lane 0 writes once the partials have met; the order statistics are written by spicey_mc_freq_ranks.
SPICEY_MEAS_HD void spicey_mc_freq_row(const SpiceyMcReduceArgs &A, int64_t k, const double *s, int64_t viol, double *freq) {
  double *dst = freq + k * (SPICEY_MC_FREQ_HEAD + A.n_rank);
  dst[0] = (double)A.n_valid; dst[1] = (double)viol; dst[2] = s[0]; dst[3] = s[1];
}

// Thread t of `threads`: the order statistics t, t + threads, ... of frequency k.
SPICEY_MEAS_HD void spicey_mc_freq_ranks(const SpiceyMcReduceArgs &A, int64_t k, const uint64_t *x, int32_t t, int32_t threads, double *freq) {
  double *dst = freq + k * (SPICEY_MC_FREQ_HEAD + A.n_rank) + SPICEY_MC_FREQ_HEAD;
  for (int32_t j = t; j < A.n_rank; j += threads) dst[j] = spicey_mc_double(x[A.ranks[j]]);
}
