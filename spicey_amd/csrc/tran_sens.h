// tran_sens.h — the host side of the sensitivities and corners of transient measurements: validation and workspace layout
// (tran_sens_exec.h holds the arithmetic and the mapping).  Plain C++, shared by spicey_abi.cpp, tran_sens.hip and the CPU
// harness of tests/tran_sens_host; the launchers of tran_sens.hip are declared at the end for translation units that have the
// HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

#include "../../include/spicey_hip.h"
#include "tran_mc.h"
#include "tran_sens_exec.h"

// The design's workspace: the record | ONE_AT_A_TIME: act [nA] int32 | step [nA] — LEVELS: tol [nE] | lvl [n_inst][nE] bytes.
struct SpiceyTsDesignLayout { int64_t off_a, off_b, total_bytes; };
inline bool spicey_ts_design_layout(int32_t mode, int32_t n_inst, int32_t nE, int32_t nA, SpiceyTsDesignLayout &l) {
  if (n_inst <= 0 || n_inst > SPICEY_MC_MAX_INST || nE <= 0 || nA < 0) return false;
  l.off_a = spicey_meas_align((int64_t)sizeof(SpiceyTsDesignArgs));
  if (mode == SPICEY_TS_LEVELS) {
    l.off_b = l.off_a + spicey_meas_align((int64_t)nE * (int64_t)sizeof(double));
    l.total_bytes = l.off_b + spicey_meas_align((int64_t)n_inst * (int64_t)nE);
  } else {
    l.off_b = l.off_a + spicey_meas_align((int64_t)(nA ? nA : 1) * (int64_t)sizeof(int32_t));
    l.total_bytes = l.off_b + spicey_meas_align((int64_t)(nA ? nA : 1) * (int64_t)sizeof(double));
  }
  return true;
}
inline int64_t spicey_ts_design_bytes(int32_t mode, int32_t n_inst, int32_t nE, int32_t nA) {
  SpiceyTsDesignLayout l;
  return spicey_ts_design_layout(mode, n_inst, nE, nA, l) ? l.total_bytes : -1;
}

// The reduction's workspace: the scalar kernel's head (tran_mc.h: spicey_tmc_layout with no probabilities) | the record |
// step [nA] | tol_act [nA].  The record's valid points into the scalar kernel's head.
struct SpiceyTsReduceLayout { SpiceyTmcLayout tmc; int64_t off_rec, off_step, off_tol, total_bytes; };
inline bool spicey_ts_reduce_layout(int32_t n_inst, int32_t n_scalar, int32_t nA, SpiceyTsReduceLayout &l) {
  if (nA < 0 || !spicey_tmc_layout(n_inst, n_scalar, 0, l.tmc)) return false;
  l.off_rec = l.tmc.total_bytes;
  l.off_step = l.off_rec + spicey_meas_align((int64_t)sizeof(SpiceyTsReduceArgs));
  l.off_tol = l.off_step + spicey_meas_align((int64_t)(nA ? nA : 1) * (int64_t)sizeof(double));
  l.total_bytes = l.off_tol + spicey_meas_align((int64_t)(nA ? nA : 1) * (int64_t)sizeof(double));
  return true;
}
inline int64_t spicey_ts_reduce_bytes(int32_t n_inst, int32_t n_scalar, int32_t nA) {
  SpiceyTsReduceLayout l;
  return spicey_ts_reduce_layout(n_inst, n_scalar, nA, l) ? l.total_bytes : -1;
}
// What serves every call (spicey_tran_sens_workspace_bytes); -1 for arguments no launch accepts.
inline int64_t spicey_ts_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t nA) {
  const int64_t a = spicey_ts_design_bytes(SPICEY_TS_ONE_AT_A_TIME, n_inst, nE, nA), b = spicey_ts_design_bytes(SPICEY_TS_LEVELS, n_inst, nE, nA);
  const int64_t c = spicey_ts_reduce_bytes(n_inst, n_scalar, nA);
  if (a < 0 || b < 0 || c < 0) return -1;
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

inline const char *spicey_ts_judge_req(const SpiceyTranSensReq *req, int32_t mode) {
  if (!req) return "null request";
  if (req->struct_bytes != (int64_t)sizeof(SpiceyTranSensReq)) return "struct_bytes is not sizeof(SpiceyTranSensReq)";
  if (req->reserved[0] != 0 || req->reserved[1] != 0) return "reserved must be 0";
  if (req->mode != SPICEY_TS_ONE_AT_A_TIME && req->mode != SPICEY_TS_LEVELS) return "unknown mode";
  if (mode >= 0 && req->mode != mode) return mode == SPICEY_TS_LEVELS ? "this call takes the LEVELS design" : "this call takes the ONE_AT_A_TIME design";
  return nullptr;
}

inline const char *spicey_ts_judge_steps(const double *step, int32_t nA) {
  for (int32_t a = 0; a < nA; a++)
    if (!std::isfinite(step[a]) || !(step[a] > 0.0 && step[a] < 1.0)) return "a step must be finite and in (0, 1)";
  return nullptr;
}
inline const char *spicey_ts_judge_tol(const double *tol, int32_t n) {
  for (int32_t e = 0; e < n; e++)
    if (!std::isfinite(tol[e]) || !(tol[e] >= 0.0 && tol[e] < 1.0)) return "a tolerance must be finite and in [0, 1)";
  return nullptr;
}

// Every refusal of a design, judged before the device is touched.  act, step, lvl and tol are HOST arrays.  mode: the design
// the entry point takes, or -1 for either.  true: `A` is the kernel's record except the pointers into the workspace.
inline bool spicey_ts_design_judge(int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C, const double *d_L,
                                   const SpiceyTranSensReq *req, int32_t mode, const int32_t *act, const double *step, const int8_t *lvl, const double *tol,
                                   double *d_oR, double *d_oC, double *d_oL, bool have_work, int64_t work_bytes, SpiceyTsDesignArgs &A, std::string &err) {
  const char *what = spicey_ts_judge_req(req, mode);
  const int64_t nE = (int64_t)nR + nC + nL;
  if (what) {
  } else if (n_inst <= 0) what = "bad counts (n_inst >= 1)";
  else if (n_inst > SPICEY_MC_MAX_INST) what = "n_inst exceeds 16384";
  else if (nR < 0 || nC < 0 || nL < 0) what = "bad counts (nR, nC, nL >= 0)";
  else if (nE == 0) what = "no element (nR + nC + nL = 0)";
  else if (nE > 0x7fffffffll) what = "too many elements";
  else if (!have_work || (nR && (!d_R || !d_oR)) || (nC && (!d_C || !d_oC)) || (nL && (!d_L || !d_oL))) what = "null buffer";
  else if (req->mode == SPICEY_TS_ONE_AT_A_TIME) {
    if (req->nA < 1) what = "ONE_AT_A_TIME needs nA >= 1";
    else if ((int64_t)n_inst != 1 + 2 * (int64_t)req->nA) what = "ONE_AT_A_TIME needs n_inst = 1 + 2 nA";
    else if (!act || !step) what = "null buffer";
    else if (work_bytes < spicey_ts_design_bytes(req->mode, n_inst, (int32_t)nE, req->nA)) what = "workspace too small (spicey_tran_sens_workspace_bytes)";
    else {
      for (int32_t a = 0; a < req->nA && !what; a++)
        if (act[a] < 0 || act[a] >= nE) what = "an active element is out of range";
        else if (a > 0 && act[a] <= act[a - 1]) what = "the active elements must be strictly ascending";
      if (!what) what = spicey_ts_judge_steps(step, req->nA);
    }
  } else {
    if (req->nA != 0) what = "LEVELS needs nA = 0";
    else if (!lvl || !tol) what = "null buffer";
    else if (work_bytes < spicey_ts_design_bytes(req->mode, n_inst, (int32_t)nE, 0)) what = "workspace too small (spicey_tran_sens_workspace_bytes)";
    else {
      what = spicey_ts_judge_tol(tol, (int32_t)nE);
      for (int64_t i = 0; i < (int64_t)n_inst * nE && !what; i++)
        if (lvl[i] < -1 || lvl[i] > 1) what = "a level must be -1, 0 or +1";
    }
  }
  if (what) {
    err = std::string("tran sens: ") + what;
    return false;
  }
  A = SpiceyTsDesignArgs{d_R, d_C, d_L, d_oR, d_oC, d_oL, nullptr, nullptr, nullptr, nullptr, n_inst, nR, nC, nL, req->nA, req->mode};
  return true;
}

// The design's workspace as the launcher uploads it and the harness reads it: `A`'s pointers set to where `base` (the
// workspace's address on the side that will read it) puts them.  head: l.total_bytes bytes.
inline void spicey_ts_design_head(const SpiceyTsDesignLayout &l, SpiceyTsDesignArgs &A, const int32_t *act, const double *step, const int8_t *lvl, const double *tol,
                                  char *head, char *base) {
  const int64_t nE = (int64_t)A.nR + A.nC + A.nL;
  memset(head, 0, (size_t)l.total_bytes);
  if (A.mode == SPICEY_TS_LEVELS) {
    A.tol = (const double *)(base + l.off_a);
    A.lvl = (const int8_t *)(base + l.off_b);
    memcpy(head + l.off_a, tol, (size_t)nE * sizeof(double));
    memcpy(head + l.off_b, lvl, (size_t)((int64_t)A.n_inst * nE));
  } else {
    A.act = (const int32_t *)(base + l.off_a);
    A.step = (const double *)(base + l.off_b);
    memcpy(head + l.off_a, act, (size_t)A.nA * sizeof(int32_t));
    memcpy(head + l.off_b, step, (size_t)A.nA * sizeof(double));
  }
  memcpy(head, &A, sizeof(A));
}

// The scalar judge of tran_mc.h under this call's prefix (no limits, no probabilities).
inline bool spicey_ts_scalar_judge(int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar, bool have_out, SpiceyTmcArgs &T,
                                   std::string &err) {
  if (!spicey_tmc_reduce_judge(n_inst, rows, scalars, n_scalar, nullptr, nullptr, nullptr, 0, have_out, INT64_MAX, T, err)) {
    err = "tran sens: " + err.substr(err.rfind("tran mc: ", 0) == 0 ? 9 : 0);
    return false;
  }
  return true;
}

// Every refusal of scalars plus reduction.  rows [3], scalars, step and tol_act are HOST data.  true: `T` is the scalar kernel's
// record and `A` the reduction's, except the pointers into the workspace, which spicey_ts_reduce_head sets.
inline bool spicey_ts_reduce_judge(int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar, const double *step, const double *tol_act,
                                   int32_t nA, bool have_out, int64_t work_bytes, SpiceyTmcArgs &T, SpiceyTsReduceArgs &A, std::string &err) {
  if (!spicey_ts_scalar_judge(n_inst, rows, scalars, n_scalar, have_out, T, err)) return false;
  const char *what = nullptr;
  if (nA < 1) what = "the reduction needs nA >= 1";
  else if ((int64_t)n_inst != 1 + 2 * (int64_t)nA) what = "the reduction needs n_inst = 1 + 2 nA";
  else if (!step || !tol_act) what = "null buffer";
  else if (work_bytes < spicey_ts_reduce_bytes(n_inst, n_scalar, nA)) what = "workspace too small (spicey_tran_sens_workspace_bytes)";
  else if (!(what = spicey_ts_judge_steps(step, nA))) what = spicey_ts_judge_tol(tol_act, nA);
  if (what) {
    err = std::string("tran sens: ") + what;
    return false;
  }
  A = SpiceyTsReduceArgs{};
  A.n_inst = n_inst; A.n_scalar = n_scalar; A.nA = nA;
  return true;
}

// The reduction's part of the workspace (behind the scalar kernel's head, which spicey_tmc_head lays out): `A`'s pointers set to
// where `base` puts them.  head: the l.total_bytes - l.off_rec bytes from l.off_rec on.
inline void spicey_ts_reduce_head(const SpiceyTsReduceLayout &l, SpiceyTsReduceArgs &A, const uint8_t *valid, const double *step, const double *tol_act, const double *x,
                                  double *sens, int8_t *sign, double *bound, char *head, char *base) {
  A.x = x; A.sens = sens; A.sign = sign; A.bound = bound;
  A.valid = valid ? (const uint8_t *)(base + l.tmc.off_valid) : nullptr;
  A.step = (const double *)(base + l.off_step);
  A.tol_act = (const double *)(base + l.off_tol);
  memset(head, 0, (size_t)(l.total_bytes - l.off_rec));
  memcpy(head, &A, sizeof(A));
  memcpy(head + (l.off_step - l.off_rec), step, (size_t)A.nA * sizeof(double));
  memcpy(head + (l.off_tol - l.off_rec), tol_act, (size_t)A.nA * sizeof(double));
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The design kernel, enqueued on `st` behind a copy of `A` (HOST, from spicey_ts_design_judge) and of the HOST arrays of its
// mode into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_ts_design(int device, const SpiceyTsDesignArgs &A, const int32_t *act, const double *step, const int8_t *lvl, const double *tol, void *d_work,
                                   hipStream_t st);
// The scalar kernel of tran_mc.hip and the reduction kernel, enqueued on `st` behind a copy of their records and of the HOST
// arrays into d_work.  d_x [n_inst][n_scalar], d_sens [n_scalar][nA][2], d_sign [n_scalar][nA], d_bound [n_scalar][8].
hipError_t spicey_launch_ts_reduce(int device, const SpiceyTmcArgs &T, const SpiceyTsReduceArgs &A, const SpiceyMcScalar *scalars, const uint8_t *valid,
                                   const double *step, const double *tol_act, double *d_x, double *d_sens, int8_t *d_sign, double *d_bound, void *d_work, hipStream_t st);
#endif
