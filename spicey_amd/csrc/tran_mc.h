// tran_mc.h — the host side of the Monte Carlo of transient runs: validation and workspace layout (tran_mc_exec.h holds the
// arithmetic and the mapping).  Plain C++, shared by spicey_abi.cpp, tran_mc.hip and the CPU harness of tests/tran_mc_host; the
// launchers of tran_mc.hip are declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

#include "../../include/spicey_hip.h"
#include "mc.h"
#include "tran_mc_exec.h"

// The draw's workspace is that of mc.h (the record | tol | icdf).  The reduction's: the record | prog [n_scalar] | valid [n_inst]
// bytes | lo [n_scalar] | hi [n_scalar] | probs [n_prob] — all of it the head, one copy from the host.
struct SpiceyTmcLayout { int64_t off_prog, off_valid, off_lo, off_hi, off_probs, total_bytes; int32_t n_pad; };
inline bool spicey_tmc_layout(int32_t n_inst, int32_t n_scalar, int32_t n_prob, SpiceyTmcLayout &l) {
  if (n_inst <= 0 || n_inst > SPICEY_MC_MAX_INST || n_scalar <= 0 || n_prob < 0) return false;
  l.n_pad = spicey_mc_pad(n_inst);
  l.off_prog = spicey_meas_align((int64_t)sizeof(SpiceyTmcArgs));
  l.off_valid = l.off_prog + spicey_meas_align((int64_t)n_scalar * (int64_t)sizeof(SpiceyMcScalar));
  l.off_lo = l.off_valid + spicey_meas_align(n_inst);
  l.off_hi = l.off_lo + spicey_meas_align((int64_t)n_scalar * (int64_t)sizeof(double));
  l.off_probs = l.off_hi + spicey_meas_align((int64_t)n_scalar * (int64_t)sizeof(double));
  l.total_bytes = l.off_probs + spicey_meas_align((int64_t)(n_prob ? n_prob : 1) * (int64_t)sizeof(double));
  return true;
}
inline int64_t spicey_tmc_reduce_bytes(int32_t n_inst, int32_t n_scalar, int32_t n_prob) {
  SpiceyTmcLayout l;
  return spicey_tmc_layout(n_inst, n_scalar, n_prob, l) ? l.total_bytes : -1;
}
// What serves either call (spicey_tran_mc_workspace_bytes); -1 for arguments no launch accepts.
inline int64_t spicey_tmc_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t log2K, int32_t n_prob) {
  const int64_t a = spicey_mc_draw_bytes(nE, log2K), b = spicey_tmc_reduce_bytes(n_inst, n_scalar, n_prob);
  return a < 0 || b < 0 ? -1 : (a > b ? a : b);
}

inline const char *spicey_tmc_judge_req(const SpiceyTranMcReq *req) {
  if (!req) return "null request";
  if (req->struct_bytes != (int64_t)sizeof(SpiceyTranMcReq)) return "struct_bytes is not sizeof(SpiceyTranMcReq)";
  if (req->reserved != 0) return "reserved must be 0";
  if (req->log2K < 0 || req->log2K > SPICEY_MC_MAX_LOG2K) return "log2K outside [0, 12]";
  return nullptr;
}

// Every refusal of a draw, judged before the device is touched: the request here, the counts, buffers, tolerances and the table
// by the judge of mc.h, whose text gets this call's prefix.  true: `A` is the kernel's record as spicey_mc_draw_judge leaves it.
inline bool spicey_tmc_draw_judge(int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C, const double *d_L, const double *tol,
                                  const double *icdf, const SpiceyTranMcReq *req, double *d_oR, double *d_oC, double *d_oL, bool have_work, int64_t work_bytes,
                                  SpiceyMcDrawArgs &A, std::string &err) {
  if (const char *what = spicey_tmc_judge_req(req)) {
    err = std::string("tran mc: ") + what;
    return false;
  }
  const int64_t need = spicey_mc_draw_bytes(nR + nC + nL, req->log2K);
  if (have_work && need >= 0 && work_bytes < need) {
    err = "tran mc: workspace too small (spicey_tran_mc_workspace_bytes)";
    return false;
  }
  const SpiceyAcMcReq ac{(int64_t)sizeof(SpiceyAcMcReq), 0, -1, req->log2K, req->keep_first, req->seed, 0};
  if (!spicey_mc_draw_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, tol, icdf, &ac, d_oR, d_oC, d_oL, have_work, work_bytes, A, err)) {
    err = "tran " + err;
    return false;
  }
  return true;
}

// One program: the text of what is wrong with it, or null.
inline const char *spicey_tmc_judge_scalar(const SpiceyMcScalar &P, const SpiceyMcRows *rows) {
  if (P.reserved != 0) return "a scalar's reserved word must be 0";
  if (P.n_ins < 1 || P.n_ins > SPICEY_MC_SCALAR_INS) return "a scalar has 1 to 48 instructions";
  int32_t depth = 0;
  for (int32_t i = 0; i < P.n_ins; i++) {
    const SpiceyMcIns &I = P.ins[i];
    if (I.op == SPICEY_MCOP_FIELD) {
      if (I.pass < 0 || I.pass >= SPICEY_TMC_N_PASS) return "a FIELD names a pass outside measure, timing, power";
      if (rows[I.pass].n_rows <= 0) return "a FIELD names a pass whose list is empty";
      if (I.row < 0 || I.row >= rows[I.pass].n_rows) return "a FIELD's row is out of range";
      if (I.field < 0 || I.field >= rows[I.pass].stride) return "a FIELD's field is out of range";
      if (spicey_mc_bits(I.c) != 0) return "an unused instruction word must be 0";
    } else if (I.op == SPICEY_MCOP_CONST) {
      if (!std::isfinite(I.c)) return "a CONST must be finite";
      if (I.pass != 0 || I.row != 0 || I.field != 0) return "an unused instruction word must be 0";
    } else if (I.op >= SPICEY_MCOP_ADD && I.op <= SPICEY_MCOP_GUARD) {
      if (I.pass != 0 || I.row != 0 || I.field != 0 || spicey_mc_bits(I.c) != 0) return "an unused instruction word must be 0";
    } else return "unknown opcode";
    const int32_t pops = I.op <= SPICEY_MCOP_CONST ? 0 : I.op == SPICEY_MCOP_GUARD ? 1 : 2, pushes = I.op == SPICEY_MCOP_GUARD ? 0 : 1;
    if (depth < pops) return "stack underflow";
    depth += pushes - pops;
    if (depth > SPICEY_MC_SCALAR_STACK) return "stack overflow (depth 4)";
  }
  return depth == 1 ? nullptr : "a scalar's program must leave exactly one value";
}

// Every refusal of a reduction.  rows [3], scalars, valid, lo, hi and probs are HOST data (the row pointers they hold are the
// device's).  true: `A` is the kernels' record except the pointers into the workspace, which spicey_tmc_head sets.
inline bool spicey_tmc_reduce_judge(int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar, const double *lo, const double *hi,
                                    const double *probs, int32_t n_prob, bool have_out, int64_t work_bytes, SpiceyTmcArgs &A, std::string &err) {
  const char *what = nullptr;
  if (n_inst <= 0 || n_scalar <= 0 || n_prob < 0) what = "bad counts (n_inst, n_scalar >= 1, n_prob >= 0)";
  else if (n_inst > SPICEY_MC_MAX_INST) what = "n_inst exceeds 16384, the keys one workgroup sorts in LDS";
  else if (n_scalar > (1 << 16) || n_prob > (1 << 16)) what = "more than 65536 scalars or probabilities";
  else if (!rows || !scalars || !have_out || (n_prob && !probs)) what = "null buffer";
  else if (work_bytes < spicey_tmc_reduce_bytes(n_inst, n_scalar, n_prob)) what = "workspace too small (spicey_tran_mc_workspace_bytes)";
  else {
    for (int p = 0; p < SPICEY_TMC_N_PASS && !what; p++)
      if (rows[p].n_rows < 0 || (rows[p].n_rows > 0 && (rows[p].stride <= 0 || !rows[p].d_rows))) what = "a pass needs n_rows >= 0 and, with rows, a stride >= 1 and a pointer";
    for (int32_t j = 0; j < n_scalar && !what; j++) what = spicey_tmc_judge_scalar(scalars[j], rows);
    for (int32_t q = 0; q < n_prob && !what; q++)
      if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) what = "a probability outside [0, 1]";
    for (int32_t j = 0; j < n_scalar && !what; j++)
      if ((lo && lo[j] != lo[j]) || (hi && hi[j] != hi[j])) what = "a limit is NaN";
  }
  if (what) {
    err = std::string("tran mc: ") + what;
    return false;
  }
  A = SpiceyTmcArgs{};
  for (int p = 0; p < SPICEY_TMC_N_PASS; p++) {
    A.rows[p] = rows[p].n_rows > 0 ? rows[p].d_rows : nullptr;
    A.n_rows[p] = rows[p].n_rows;
    A.stride[p] = rows[p].n_rows > 0 ? rows[p].stride : 0;
  }
  A.n_inst = n_inst; A.n_pad = spicey_mc_pad(n_inst); A.n_scalar = n_scalar; A.n_prob = n_prob; A.sort_threads = spicey_mc_sort_threads(A.n_pad);
  return true;
}

// The reduction's workspace as the launcher uploads it and the harness reads it: `A`'s pointers set to where `base` (the
// workspace's address on the side that will read it) puts them.  head: l.total_bytes bytes.  x: the side's [n_inst][n_scalar].
inline void spicey_tmc_head(const SpiceyTmcLayout &l, SpiceyTmcArgs &A, const SpiceyMcScalar *scalars, const uint8_t *valid, const double *lo, const double *hi,
                            const double *probs, double *x, char *head, char *base) {
  const double inf = INFINITY;
  A.prog = (const SpiceyMcScalar *)(base + l.off_prog);
  A.valid = valid ? (const uint8_t *)(base + l.off_valid) : nullptr;
  A.lo = (const double *)(base + l.off_lo);
  A.hi = (const double *)(base + l.off_hi);
  A.probs = (const double *)(base + l.off_probs);
  A.x = x;
  memset(head, 0, (size_t)l.total_bytes);
  memcpy(head, &A, sizeof(A));
  memcpy(head + l.off_prog, scalars, (size_t)A.n_scalar * sizeof(SpiceyMcScalar));
  if (valid) memcpy(head + l.off_valid, valid, (size_t)A.n_inst);
  for (int32_t j = 0; j < A.n_scalar; j++) {
    const double a = lo ? lo[j] : -inf, b = hi ? hi[j] : inf;
    memcpy(head + l.off_lo + (int64_t)j * 8, &a, 8);
    memcpy(head + l.off_hi + (int64_t)j * 8, &b, 8);
  }
  if (A.n_prob) memcpy(head + l.off_probs, probs, (size_t)A.n_prob * sizeof(double));
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The draw kernel, enqueued on `st` behind a copy of `A` (HOST, from spicey_tmc_draw_judge), tol (HOST [nE]) and icdf (HOST
// [K + 1]) into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_tmc_draw(int device, const SpiceyMcDrawArgs &A, const double *tol, const double *icdf, void *d_work, hipStream_t st);
// The scalar kernel alone, enqueued on `st` behind a copy of `A` and of the HOST arrays into d_work: d_x [n_inst][n_scalar] (what
// spicey_launch_tmc_reduce runs first; tran_sens.hip runs it on its own).
hipError_t spicey_launch_tmc_scalars(int device, const SpiceyTmcArgs &A, const SpiceyMcScalar *scalars, const uint8_t *valid, const double *lo, const double *hi,
                                     const double *probs, double *d_x, void *d_work, hipStream_t st);
// The three kernels of the reduction, enqueued on `st` behind a copy of `A` (HOST, from spicey_tmc_reduce_judge) and of the HOST
// arrays into d_work.  d_x [n_inst][n_scalar], d_stat [n_scalar][8 + 2 n_prob], d_sample [n_inst][2] int64.
hipError_t spicey_launch_tmc_reduce(int device, const SpiceyTmcArgs &A, const SpiceyMcScalar *scalars, const uint8_t *valid, const double *lo, const double *hi,
                                    const double *probs, double *d_x, double *d_stat, int64_t *d_sample, void *d_work, hipStream_t st);
#endif
