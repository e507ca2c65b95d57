// tran_mc_exec.h — Monte Carlo of transient runs: the one definition of the draw into a transient run's value arrays, of the
// scalar programs over measurement rows and of the reduction across instances, used by the kernels of tran_mc.hip and by the
// CPU harness of tests/tran_mc_host (compiled without FMA contraction on both sides, so the two give the same bits).
//
// The draw.  That of mc_exec.h — same counter, key, table and operations (spicey_mc_uniform, spicey_mc_deviate) — except for the
// resistor's last step: the transient kernels form 1.0 / R themselves, so the resistor array gets R g in ohms.
//
// Scalars.  One thread per (scalar j, sample s), the sample the fast index, runs the scalar's program, at most 48 instructions over a stack of at most 4
// doubles (spicey_hip.h: SpiceyMcScalar), on the sample's rows of the fixed-row passes — measure, timing, power —; every
// arithmetic instruction is one rounded operation.  GUARD pops g and, if !(g >= 0), makes the scalar NaN whatever else the
// program computes.  A NaN result is stored as the one quiet NaN 0x7ff8000000000000, so x [n_inst][n_scalar] is a function of
// the rows alone (the sign of a NaN that 0.0 / 0.0 gives differs between machines); an invalid sample's x is that NaN too.
//
// The reduction.  Per sample one thread: the scalars it violates, !(x >= lo[j] && x <= hi[j]) — a NaN violates —, and the lowest
// such j.  Per scalar one workgroup: the keys of x[.][j] — with u = bits(x): ~u if the sign bit is set, else u | 1 << 63; any NaN
// 0xffff...fe; an invalid sample and the padding 0xffff...ff, so -inf < ... < -0 < +0 < ... < +inf < NaN < invalid as unsigned
// integers — sorted in LDS by the bitonic network of mc_exec.h (spicey_mc_sort); n_valid and n_num (valid and not NaN) by binary
// search in the sorted keys; then 64 lanes: lane l adds x[l], x[l + 64], ... of the first n_num decoded values to +0.0, once as
// they are and once squared, counts the violations among the first n_valid and keeps the lowest sample index whose key equals
// the first and the n_num-th sorted key; the lanes meet by s[l] += s[l + stride], stride 32 .. 1 (integers by + and min).  Per
// probability p the ranks r = (int64)(p (double)(n_num - 1)) and min(r + 1, n_num - 1) are formed here: n_num is known only here.
//   d_stat [n_scalar][8 + 2 n_prob] = {n_valid, n_num, n_viol, sum x, sum x x, s_min, s_max, 0, q_(r0), q_(r0 + 1), q_(r1), ...}
// With n_num = 0 the sums are +0.0, the indices -1 and the order statistics NaN.  Apart from the two sums nothing is a
// floating-point accumulation and no floating-point comparison orders anything: the result does not depend on the thread count.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mc_exec.h"

#define SPICEY_TMC_STAT_HEAD 8     // doubles of a d_stat row before the order statistics
#define SPICEY_TMC_N_PASS 3        // the fixed-row passes a FIELD names: measure, timing, power
#define SPICEY_TMC_NAN_KEY 0xfffffffffffffffeull
#define SPICEY_TMC_NAN_BITS 0x7ff8000000000000ull

// A validated reduction with the buffers it runs on (tran_mc.h: spicey_tmc_reduce_judge).  prog, valid, lo, hi and probs lie in
// the workspace; valid is null when every sample is valid.
struct SpiceyTmcArgs {
  const double *rows[SPICEY_TMC_N_PASS];  // [n_inst][n_rows][stride] per pass (null: the pass has no rows)
  const SpiceyMcScalar *prog;             // [n_scalar]
  const uint8_t *valid;                   // [n_inst]
  const double *lo, *hi;                  // [n_scalar], -inf / +inf where there is no limit
  const double *probs;                    // [n_prob]
  double *x;                              // [n_inst][n_scalar]
  int32_t n_rows[SPICEY_TMC_N_PASS], stride[SPICEY_TMC_N_PASS];
  int32_t n_inst, n_pad, n_scalar, n_prob, sort_threads;
};

// Thread idx = s * nE + e of the draw: spicey_mc_draw with the resistor left in ohms.
SPICEY_MEAS_HD void spicey_tmc_draw(const SpiceyMcDrawArgs &A, int64_t idx) {
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
    A.oR[at] = A.R[at] * g;
  } else if (e < A.nR + A.nC) {
    const int64_t at = s * A.nC + (e - A.nR);
    A.oC[at] = A.C[at] * g;
  } else {
    const int64_t at = s * A.nL + (e - A.nR - A.nC);
    A.oL[at] = A.L[at] * g;
  }
}

SPICEY_MEAS_HD bool spicey_tmc_ok(const SpiceyTmcArgs &A, int64_t s) { return s < A.n_inst && (!A.valid || A.valid[s]); }

// The value of scalar j of (valid) sample s.  The program was judged: no stack check here.
SPICEY_MEAS_HD double spicey_tmc_eval(const SpiceyTmcArgs &A, int64_t s, int32_t j) {
  const SpiceyMcScalar &P = A.prog[j];
  // (the stack as four named values with its top in t0: nothing is indexed by a run-time number, so nothing leaves registers)
  static_assert(SPICEY_MC_SCALAR_STACK == 4, "the stack is four named values");
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  bool bad = false;
  for (int32_t i = 0; i < P.n_ins; i++) {
    const SpiceyMcIns I = P.ins[i];
    if (I.op == SPICEY_MCOP_FIELD || I.op == SPICEY_MCOP_CONST) {
      double v = I.c;
      // (A is the record in the workspace itself, not a copy: the pass indexes memory, not registers)
      if (I.op == SPICEY_MCOP_FIELD) v = A.rows[I.pass][((int64_t)s * A.n_rows[I.pass] + I.row) * A.stride[I.pass] + I.field];
      t3 = t2; t2 = t1; t1 = t0; t0 = v;
    } else if (I.op == SPICEY_MCOP_GUARD) {
      if (!(t0 >= 0.0)) bad = true;
      t0 = t1; t1 = t2; t2 = t3;
    } else {
      const double b = t0, a = t1;
      t0 = I.op == SPICEY_MCOP_ADD ? a + b : I.op == SPICEY_MCOP_SUB ? a - b : I.op == SPICEY_MCOP_MUL ? a * b : a / b;
      t1 = t2; t2 = t3;
    }
  }
  return (bad || t0 != t0) ? spicey_mc_double(SPICEY_TMC_NAN_BITS) : t0;
}

// Thread idx = j * n_inst + s of the scalar kernel: the sample is the fast index, so the lanes of a wave run one program
// (except where a scalar's samples end) — no divergence on the opcodes, one record fetched per wave — on neighbouring samples.
SPICEY_MEAS_HD void spicey_tmc_scalar(const SpiceyTmcArgs &A, int64_t idx) {
  const int32_t j = (int32_t)(idx / A.n_inst);
  const int64_t s = idx - (int64_t)j * A.n_inst;
  A.x[s * A.n_scalar + j] = spicey_tmc_ok(A, s) ? spicey_tmc_eval(A, s, j) : spicey_mc_double(SPICEY_TMC_NAN_BITS);
}

SPICEY_MEAS_HD bool spicey_tmc_violates(const SpiceyTmcArgs &A, int32_t j, double x) { return !(x >= A.lo[j] && x <= A.hi[j]); }

// Thread s of the per-sample kernel: d_sample [n_inst][2] = {scalars the sample violates, the lowest such j or -1}.
SPICEY_MEAS_HD void spicey_tmc_sample(const SpiceyTmcArgs &A, int64_t s, int64_t *sample) {
  int64_t n = -1, f = -1;
  if (spicey_tmc_ok(A, s)) {
    n = 0;
    for (int32_t j = 0; j < A.n_scalar; j++)
      if (spicey_tmc_violates(A, j, A.x[s * A.n_scalar + j])) {
        n++;
        if (f < 0) f = j;
      }
  }
  sample[2 * s] = n;
  sample[2 * s + 1] = f;
}

// The key that orders every double as an unsigned integer (file text).
SPICEY_MEAS_HD uint64_t spicey_tmc_key(double x) {
  const uint64_t u = spicey_mc_bits(x);
  if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return SPICEY_TMC_NAN_KEY;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
SPICEY_MEAS_HD double spicey_tmc_unkey(uint64_t k) {
  if (k >= SPICEY_TMC_NAN_KEY) return spicey_mc_double(SPICEY_TMC_NAN_BITS);
  return spicey_mc_double((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// The key of sample s < n_pad of scalar j: what the workgroup of j loads before it sorts.
SPICEY_MEAS_HD uint64_t spicey_tmc_key_of(const SpiceyTmcArgs &A, int64_t s, int32_t j) {
  return spicey_tmc_ok(A, s) ? spicey_tmc_key(A.x[s * A.n_scalar + j]) : SPICEY_MC_PAD_KEY;
}

// The number of sorted keys below `bound` (every thread asks for itself: log2(n_pad) + 1 reads).
SPICEY_MEAS_HD int32_t spicey_tmc_count_below(const uint64_t *x, int32_t n_pad, uint64_t bound) {
  int32_t lo = 0, hi = n_pad;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (x[mid] < bound) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// What lane `lane` of the summing wave brings: its sums, its violations, and its lowest samples with the extreme keys.
struct SpiceyTmcPartial { double s0, s1; int64_t viol, s_min, s_max; };

SPICEY_MEAS_HD void spicey_tmc_stat_lane(const SpiceyTmcArgs &A, int32_t j, const uint64_t *x, int32_t n_valid, int32_t n_num, int32_t lane, SpiceyTmcPartial *p) {
  const int64_t none = 0x7fffffffffffffffll;
  p->s0 = 0.0; p->s1 = 0.0; p->viol = 0; p->s_min = none; p->s_max = none;
  for (int32_t i = lane; i < n_num; i += SPICEY_MC_LANES) {
    const double v = spicey_tmc_unkey(x[i]);
    p->s0 = p->s0 + v;
    p->s1 = p->s1 + v * v;
  }
  for (int32_t i = lane; i < n_valid; i += SPICEY_MC_LANES) p->viol += spicey_tmc_violates(A, j, spicey_tmc_unkey(x[i])) ? 1 : 0;
  if (n_num > 0) {
    const uint64_t k_min = x[0], k_max = x[n_num - 1];
    for (int32_t s = lane; s < A.n_inst; s += SPICEY_MC_LANES) {
      const uint64_t k = spicey_tmc_key_of(A, s, j);
      if (k == k_min && s < p->s_min) p->s_min = s;
      if (k == k_max && s < p->s_max) p->s_max = s;
    }
  }
}

// How lane l takes lane l + stride's partial.
SPICEY_MEAS_HD void spicey_tmc_stat_meet(SpiceyTmcPartial *p, const SpiceyTmcPartial &q) {
  p->s0 = p->s0 + q.s0;
  p->s1 = p->s1 + q.s1;
  p->viol += q.viol;
  if (q.s_min < p->s_min) p->s_min = q.s_min;
  if (q.s_max < p->s_max) p->s_max = q.s_max;
}

// What lane 0 writes once the partials have met; the order statistics are written by spicey_tmc_stat_ranks.
SPICEY_MEAS_HD void spicey_tmc_stat_row(const SpiceyTmcArgs &A, int32_t j, int32_t n_valid, int32_t n_num, const SpiceyTmcPartial &p, double *stat) {
  double *dst = stat + (int64_t)j * (SPICEY_TMC_STAT_HEAD + 2 * A.n_prob);
  dst[0] = (double)n_valid; dst[1] = (double)n_num; dst[2] = (double)p.viol; dst[3] = p.s0; dst[4] = p.s1;
  dst[5] = n_num > 0 ? (double)p.s_min : -1.0;
  dst[6] = n_num > 0 ? (double)p.s_max : -1.0;
  dst[7] = 0.0;
}

// Thread t of `threads`: the order statistics of probabilities t, t + threads, ... of scalar j.
SPICEY_MEAS_HD void spicey_tmc_stat_ranks(const SpiceyTmcArgs &A, int32_t j, const uint64_t *x, int32_t n_num, int32_t t, int32_t threads, double *stat) {
  double *dst = stat + (int64_t)j * (SPICEY_TMC_STAT_HEAD + 2 * A.n_prob) + SPICEY_TMC_STAT_HEAD;
  for (int32_t q = t; q < A.n_prob; q += threads) {
    double a = spicey_mc_double(SPICEY_TMC_NAN_BITS), b = a;
    if (n_num > 0) {
      const int64_t r = (int64_t)(A.probs[q] * (double)(n_num - 1));
      const int64_t r1 = r + 1 < n_num ? r + 1 : n_num - 1;
      a = spicey_tmc_unkey(x[r]);
      b = spicey_tmc_unkey(x[r1]);
    }
    dst[2 * q] = a;
    dst[2 * q + 1] = b;
  }
}
