// spectrum_exec.h — the spectrum of a transient's waveforms (what SPICE calls fft / spec): the one definition of the
// arithmetic and of the workgroup's thread and stage mapping, used by the kernel of spectrum.hip and by the CPU harness of
// tests/spectrum_host (compiled without FMA contraction on both sides, so the two give the same bits).
//
// A request (SpiceySpecReq, include/spicey_hip.h) names one signal x_j = a[inst][step_from + j][col] (minus
// a[inst][step_from + j][col_ref], one rounded subtraction, when col_ref >= 0) of out_v or out_i, N = 2^log2n samples of
// it, a window, a band of bins and a kind.  One workgroup of `threads` threads (a power of two) takes one (instance,
// request) item through these phases, a barrier behind each:
//   load     thread t takes the samples j = t, t + threads, ...: y_j = x_j w_j (one rounded product; none for the
//            rectangular window) goes to slot bitrev(j) of the real plane, 0.0 to that slot of the imaginary plane;
//   stages   s = 0 .. log2n - 1, h = 2^s: thread t takes the butterflies b = t, t + threads, ... < N/2 with j = b mod h,
//            g = b div h, i = 2h g + j, W = T[j N / (2h)]:
//              tr = b.re W.re - b.im W.im,  ti = b.re W.im + b.im W.re,  z[i] = a + t,  z[i+h] = a - t
//            every product, sum and difference rounded on its own.  A butterfly reads and writes its own two slots only, so
//            the assignment of butterflies to threads changes no bit;
//   result   kind 0: element e = t, t + threads, ... of the row is re / im of bin bin_from + e div 2, 0.0 behind the band;
//            kind 1: thread t scans the bins bin_from + t, + threads, ... in ascending order with `P > best` from best =
//            0.0, the threads' candidates meet in a tree — the better of two is the one with the larger P, on equal P the
//            one with the lower bin: a total order, so the winner is the FIRST largest bin of the band whatever the tree
//            looks like — and the row's 8 doubles (0.0 behind them) are written from the planes.
// The planes are split: re[N] then im[N], 16 N bytes; the tree's candidates live in 2 x `threads` slots beside them.
#pragma once
#include <stdint.h>

#include "measure_exec.h"  // SPICEY_MEAS_HD, SPICEY_MEAS_THREADS, SPICEY_MEAS_HEAD_ALIGN

#define SPICEY_SPEC_HD SPICEY_MEAS_HD
#define SPICEY_SPEC_THREADS SPICEY_MEAS_THREADS
#define SPICEY_SPEC_DOM_DOUBLES 8  // a kind 1 row

// A validated request as the kernel reads it, in the caller's order (row r of the result is request r): tw_off / win_off
// are the places, in doubles, of its twiddle table T[N/2][2] = {re, im} and of its window table w[N] in the table area
// (win_off = -1: rectangular, no product).
struct SpiceySpecDevReq {
  int32_t signal, col, col_ref, kind;
  int64_t step_from;
  int32_t log2n, window, bin_from, bin_to;
  int64_t tw_off, win_off;
};

// j's log2n bits in reverse order
SPICEY_SPEC_HD int32_t spicey_spec_bitrev(int32_t j, int32_t log2n) {
  int32_t r = 0;
  for (int32_t b = 0; b < log2n; b++) r |= ((j >> b) & 1) << (log2n - 1 - b);
  return r;
}

// P_k from the planes; -1.0 for a bin outside 0 .. N/2
SPICEY_SPEC_HD double spicey_spec_power(const double *re, const double *im, int32_t k, int32_t half) {
  if (k < 0 || k > half) return -1.0;
  const double a = re[k] * re[k], b = im[k] * im[k];
  return a + b;
}

// candidate (pa, ka) against (pb, kb): true if b is the better one.  k = -1 (no bin won: P = 0.0) loses to every winner,
// whose P is > 0.0.
SPICEY_SPEC_HD bool spicey_spec_better(double pa, int32_t ka, double pb, int32_t kb) {
  return pb > pa || (pb == pa && kb >= 0 && (ka < 0 || kb < ka));
}

// One (instance, request) item by a workgroup of `threads` threads.  par(f) runs f(t) for every thread t of the workgroup
// and ends with a barrier: the kernel's is { f(threadIdx.x); __syncthreads(); }, the harness's a loop over t.  x: the
// signal's column(s) at the instance's step 0, stride n doubles per step.  re / im: the planes, N doubles each; cand_p /
// cand_k: `threads` slots each.  row: the item's row of the result, out_stride doubles.
template <class Par>
SPICEY_SPEC_HD void spicey_spec_item(Par par, int32_t threads, const SpiceySpecDevReq &q, const double *tables, const double *base, int64_t n, double *re, double *im,
                                     double *cand_p, int32_t *cand_k, double *row, int32_t out_stride) {
  const int32_t N = 1 << q.log2n, half = N >> 1;
  const double *T = tables + q.tw_off;
  const double *w = q.win_off >= 0 ? tables + q.win_off : nullptr;
  const double *pa = base + q.step_from * n + q.col;
  const double *pb = q.col_ref >= 0 ? base + q.step_from * n + q.col_ref : nullptr;
  par([&](int32_t t) {
    for (int32_t j = t; j < N; j += threads) {
      double x = pa[(int64_t)j * n];
      if (pb) x = x - pb[(int64_t)j * n];
      if (w) x = x * w[j];
      const int32_t slot = spicey_spec_bitrev(j, q.log2n);
      re[slot] = x;
      im[slot] = 0.0;
    }
  });
  for (int32_t s = 0; s < q.log2n; s++) {
    const int32_t h = 1 << s, tw_shift = q.log2n - 1 - s;
    par([&](int32_t t) {
      for (int32_t b = t; b < half; b += threads) {
        const int32_t j = b & (h - 1);
        const int32_t i = ((b >> s) << (s + 1)) + j;
        const double wr = T[2 * ((int64_t)j << tw_shift)], wi = T[2 * ((int64_t)j << tw_shift) + 1];
        const double ar = re[i], ai = im[i], br = re[i + h], bi = im[i + h];
        const double p0 = br * wr, p1 = bi * wi, p2 = br * wi, p3 = bi * wr;
        const double tr = p0 - p1, ti = p2 + p3;
        re[i] = ar + tr;
        im[i] = ai + ti;
        re[i + h] = ar - tr;
        im[i + h] = ai - ti;
      }
    });
  }
  if (q.kind == 0) {
    const int32_t len = 2 * (q.bin_to - q.bin_from + 1);
    par([&](int32_t t) {
      for (int32_t e = t; e < out_stride; e += threads) {
        const int32_t k = q.bin_from + (e >> 1);
        row[e] = e < len ? ((e & 1) ? im[k] : re[k]) : 0.0;
      }
    });
    return;
  }
  par([&](int32_t t) {
    double best = 0.0;
    int32_t kb = -1;
    for (int32_t k = q.bin_from + t; k <= q.bin_to; k += threads) {
      const double p = spicey_spec_power(re, im, k, half);
      if (p > best) { best = p; kb = k; }
    }
    cand_p[t] = best;
    cand_k[t] = kb;
  });
  for (int32_t d = threads >> 1; d > 0; d >>= 1)
    par([&](int32_t t) {
      if (t < d && spicey_spec_better(cand_p[t], cand_k[t], cand_p[t + d], cand_k[t + d])) {
        cand_p[t] = cand_p[t + d];
        cand_k[t] = cand_k[t + d];
      }
    });
  par([&](int32_t t) {
    const int32_t k = cand_k[0];
    for (int32_t e = t; e < out_stride; e += threads) {
      double v = 0.0;
      if (k < 0) v = e == 0 ? -1.0 : 0.0;
      else if (e == 0) v = (double)k;
      else if (e == 1) v = re[k];
      else if (e == 2) v = im[k];
      else if (e <= 5) v = spicey_spec_power(re, im, k + e - 4, half);
      row[e] = v;
    }
  });
}

// Doubles of a request's own row
SPICEY_SPEC_HD int32_t spicey_spec_row_doubles(int32_t kind, int32_t bin_from, int32_t bin_to) {
  return kind == 0 ? 2 * (bin_to - bin_from + 1) : SPICEY_SPEC_DOM_DOUBLES;
}
