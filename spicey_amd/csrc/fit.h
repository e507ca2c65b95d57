// fit.h — the host side of sizing elements to measured goals: validation and workspace layout (fit_exec.h holds the arithmetic,
// the mapping and the order).  Plain C++, shared by fit_abi.cpp, fit.hip and the CPU harness of tests/fit_host; the launchers
// of fit.hip are declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spicey_hip.h"
#include "fit_exec.h"

#define SPICEY_FIT_MAX_INST 16384  // the scalar kernel's own bound (tran_mc.h)

inline int64_t spicey_fit_align(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
// Bytes of dynamic LDS of the update: the matrix with its right-hand side, row stride nA + 1 doubles (132 096 at nA = 128).
inline size_t spicey_fit_lds_bytes(int32_t nA) { return (size_t)nA * (size_t)(nA + 1) * sizeof(double); }

// The workspace: the design's head — record | step [nA] | act [nA] —, the update's head — record | step [nA] | g_lo | g_hi
// [n_ckt][nA] | goals [n_ckt][n_scalar] | valid [n_inst] — and the circuits' state, which no launch uploads.  The design's part
// does not depend on n_scalar.
struct SpiceyFitLayout { int64_t off_dstep, off_act, off_rec, off_step, off_lo, off_hi, off_goals, off_valid, off_state, total_bytes, n_inst; };
inline bool spicey_fit_layout(int32_t n_ckt, int32_t nA, int32_t n_scalar, SpiceyFitLayout &l) {
  if (n_ckt < 1 || nA < 1 || nA > SPICEY_FIT_MAX_NA || n_scalar < 1) return false;
  l.n_inst = (int64_t)n_ckt * (1 + 2 * nA);
  if (l.n_inst > SPICEY_FIT_MAX_INST) return false;
  const int64_t per = spicey_fit_align((int64_t)n_ckt * nA * (int64_t)sizeof(double)), vec = spicey_fit_align((int64_t)nA * (int64_t)sizeof(double));
  l.off_dstep = spicey_fit_align((int64_t)sizeof(SpiceyFitArgs));
  l.off_act = l.off_dstep + vec;
  l.off_rec = l.off_act + spicey_fit_align((int64_t)nA * (int64_t)sizeof(int32_t));
  l.off_step = l.off_rec + spicey_fit_align((int64_t)sizeof(SpiceyFitArgs));
  l.off_lo = l.off_step + vec;
  l.off_hi = l.off_lo + per;
  l.off_goals = l.off_hi + per;
  l.off_valid = l.off_goals + spicey_fit_align((int64_t)n_ckt * n_scalar * (int64_t)sizeof(SpiceyFitGoal));
  l.off_state = l.off_valid + spicey_fit_align(l.n_inst);
  l.total_bytes = l.off_state + spicey_fit_align((int64_t)n_ckt * spicey_fit_state_doubles(nA) * (int64_t)sizeof(double));
  return true;
}
inline int64_t spicey_fit_bytes(int32_t n_ckt, int32_t nA, int32_t n_scalar) {
  SpiceyFitLayout l;
  return spicey_fit_layout(n_ckt, nA, n_scalar, l) ? l.total_bytes : -1;
}

inline bool spicey_fit_pos(double v) { return std::isfinite(v) && v > 0.0; }
inline bool spicey_fit_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// Every refusal of the request, judged before the device is touched.  run: spicey_run_fit, which looks at max_iter.
inline const char *spicey_fit_judge_req(const SpiceyFitReq *req, bool run) {
  if (!req) return "null request";
  if (req->struct_bytes != (int64_t)sizeof(SpiceyFitReq)) return "struct_bytes is not sizeof(SpiceyFitReq)";
  if (req->pad != 0 || req->reserved != 0) return "pad and reserved must be 0";
  if (req->n_ckt < 1) return "bad counts (n_ckt >= 1)";
  if (req->nA < 1) return "bad counts (nA >= 1)";
  if (req->nA > SPICEY_FIT_MAX_NA) return "nA exceeds 128, the columns of the matrix the update keeps in LDS";
  if ((int64_t)req->n_ckt * (1 + 2 * (int64_t)req->nA) > SPICEY_FIT_MAX_INST) return "n_inst = n_ckt (1 + 2 nA) exceeds 16384";
  if (run && req->max_iter < 1) return "max_iter must be >= 1";
  if (!spicey_fit_nonneg(req->lambda0)) return "lambda0 must be finite and >= 0";
  if (!(std::isfinite(req->lam_up) && req->lam_up > 1.0)) return "lam_up must be finite and > 1";
  if (!(req->lam_down > 0.0 && req->lam_down <= 1.0)) return "lam_down must be in (0, 1]";
  if (!(std::isfinite(req->lam_max) && req->lam_max >= req->lambda0)) return "lam_max must be finite and >= lambda0";
  if (!spicey_fit_pos(req->max_step)) return "max_step must be finite and > 0";
  if (!spicey_fit_nonneg(req->x_tol) || !spicey_fit_nonneg(req->f_tol)) return "x_tol and f_tol must be finite and >= 0";
  if (!spicey_fit_pos(req->pivot_min)) return "pivot_min must be finite and > 0";
  return nullptr;
}
inline const char *spicey_fit_judge_steps(const double *step, int32_t nA) {
  for (int32_t a = 0; a < nA; a++)
    if (!std::isfinite(step[a]) || !(step[a] > 0.0 && step[a] < 1.0)) return "a step must be finite and in (0, 1)";
  return nullptr;
}

// Every refusal of a design.  act and step are HOST arrays.  true: `A` is the kernel's record except the pointers into the
// workspace, which spicey_fit_design_head sets.
inline bool spicey_fit_design_judge(int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C, const double *d_L, const SpiceyFitReq *req,
                                    const int32_t *act, const double *step, const double *d_g, double *d_oR, double *d_oC, double *d_oL, bool have_work,
                                    int64_t work_bytes, SpiceyFitArgs &A, std::string &err) {
  const char *what = spicey_fit_judge_req(req, false);
  SpiceyFitLayout l{};
  const int64_t nE = (int64_t)nR + nC + nL;
  if (what) {
  } else if (nR < 0 || nC < 0 || nL < 0) what = "bad counts (nR, nC, nL >= 0)";
  else if (nE == 0) what = "no element (nR + nC + nL = 0)";
  else if (nE > 0x7fffffffll || (int64_t)req->n_ckt * (1 + 2 * (int64_t)req->nA) * nE > 0x7fffffffll) return err = "fit: too many elements", false;
  else if (req->nA > nE) what = "more active elements than elements";
  else if (!have_work || !act || !step || !d_g || (nR && (!d_R || !d_oR)) || (nC && (!d_C || !d_oC)) || (nL && (!d_L || !d_oL))) what = "null buffer";
  else if (!spicey_fit_layout(req->n_ckt, req->nA, 1, l) || work_bytes < l.off_rec) what = "workspace too small (spicey_fit_workspace_bytes)";
  else {
    for (int32_t a = 0; a < req->nA && !what; a++)
      if (act[a] < 0 || act[a] >= nE) what = "an active element is out of range";
      else if (a > 0 && act[a] <= act[a - 1]) what = "the active elements must be strictly ascending";
    if (!what) what = spicey_fit_judge_steps(step, req->nA);
  }
  if (what) {
    err = std::string("fit: ") + what;
    return false;
  }
  A = SpiceyFitArgs{};
  A.R = d_R; A.C = d_C; A.L = d_L; A.oR = d_oR; A.oC = d_oC; A.oL = d_oL; A.g = const_cast<double *>(d_g);
  A.n_ckt = req->n_ckt; A.nA = req->nA; A.nR = nR; A.nC = nC; A.nL = nL; A.n_scalar = 1;
  return true;
}

// The design's head (l.off_rec bytes) as the launcher uploads it and the harness reads it: `A`'s pointers set to where `base` (the
// workspace's address on the side that will read it) puts them.  l: of any n_scalar.
inline void spicey_fit_design_head(const SpiceyFitLayout &l, SpiceyFitArgs &A, const int32_t *act, const double *step, char *head, char *base) {
  A.step = (const double *)(base + l.off_dstep);
  A.act = (const int32_t *)(base + l.off_act);
  memset(head, 0, (size_t)l.off_rec);
  memcpy(head, &A, sizeof(A));
  memcpy(head + l.off_dstep, step, (size_t)A.nA * sizeof(double));
  memcpy(head + l.off_act, act, (size_t)A.nA * sizeof(int32_t));
}

inline const char *spicey_fit_judge_goal(const SpiceyFitGoal &G) {
  if (G.pad != 0) return "a goal's pad must be 0";
  if (G.kind < SPICEY_FIT_EQ || G.kind > SPICEY_FIT_BETWEEN) return "unknown goal kind";
  if (!spicey_fit_pos(G.weight)) return "a weight must be finite and > 0";
  if (G.kind != SPICEY_FIT_AT_MOST && !std::isfinite(G.lo)) return "a goal's bound must be finite";
  if ((G.kind == SPICEY_FIT_AT_MOST || G.kind == SPICEY_FIT_BETWEEN) && !std::isfinite(G.hi)) return "a goal's bound must be finite";
  if (G.kind == SPICEY_FIT_BETWEEN && G.lo > G.hi) return "a BETWEEN goal needs lo <= hi";
  return nullptr;
}

// Every refusal of an update.  step, g_lo, g_hi, goals and valid are HOST arrays.  true: `A` is the kernel's record except the
// pointers into the workspace, which spicey_fit_update_head sets.
inline bool spicey_fit_update_judge(const SpiceyFitReq *req, int32_t n_scalar, int32_t first, const double *step, const double *g_lo, const double *g_hi,
                                    const SpiceyFitGoal *goals, const double *d_x, double *d_g, double *d_rows, int32_t *d_done, bool have_work, int64_t work_bytes,
                                    SpiceyFitArgs &A, std::string &err) {
  const char *what = spicey_fit_judge_req(req, false);
  SpiceyFitLayout l{};
  if (what) {
  } else if (n_scalar < 1) what = "bad counts (n_scalar >= 1)";
  else if (n_scalar > (1 << 16)) what = "more than 65536 scalars";
  else if (!have_work || !step || !g_lo || !g_hi || !goals || !d_x || !d_g || !d_rows || !d_done) what = "null buffer";
  else if (!spicey_fit_layout(req->n_ckt, req->nA, n_scalar, l) || work_bytes < l.total_bytes) what = "workspace too small (spicey_fit_workspace_bytes)";
  else {
    what = spicey_fit_judge_steps(step, req->nA);
    for (int64_t i = 0; i < (int64_t)req->n_ckt * req->nA && !what; i++)
      if (!(std::isfinite(g_lo[i]) && std::isfinite(g_hi[i]) && g_lo[i] > 0.0 && g_lo[i] <= g_hi[i])) what = "the bounds must be finite with 0 < g_lo <= g_hi";
    for (int64_t i = 0; i < (int64_t)req->n_ckt * n_scalar && !what; i++) what = spicey_fit_judge_goal(goals[i]);
  }
  if (what) {
    err = std::string("fit: ") + what;
    return false;
  }
  A = SpiceyFitArgs{};
  A.g = d_g; A.x = d_x; A.rows = d_rows; A.done = d_done;
  A.lambda0 = req->lambda0; A.lam_up = req->lam_up; A.lam_down = req->lam_down; A.lam_max = req->lam_max; A.max_step = req->max_step;
  A.x_tol = req->x_tol; A.f_tol = req->f_tol; A.pivot_min = req->pivot_min;
  A.n_ckt = req->n_ckt; A.nA = req->nA; A.n_scalar = n_scalar; A.first = first != 0;
  return true;
}

// `A`'s pointers into the workspace, set to where `base` (the workspace's address on the side that will read it) puts them.
inline void spicey_fit_update_pointers(const SpiceyFitLayout &l, SpiceyFitArgs &A, bool have_valid, char *base) {
  A.step = (const double *)(base + l.off_step);
  A.g_lo = (const double *)(base + l.off_lo);
  A.g_hi = (const double *)(base + l.off_hi);
  A.goals = (const SpiceyFitGoal *)(base + l.off_goals);
  A.valid = have_valid ? (const uint8_t *)(base + l.off_valid) : nullptr;
  A.state = (double *)(base + l.off_state);
}
// The update's head (l.off_state - l.off_rec bytes from l.off_rec on): the record with its pointers set and the HOST arrays.
inline void spicey_fit_update_head(const SpiceyFitLayout &l, SpiceyFitArgs &A, const double *step, const double *g_lo, const double *g_hi, const SpiceyFitGoal *goals,
                                   const uint8_t *valid, char *head, char *base) {
  const size_t n = (size_t)A.n_ckt * (size_t)A.nA;
  const int64_t o = l.off_rec;
  spicey_fit_update_pointers(l, A, valid != nullptr, base);
  memset(head, 0, (size_t)(l.off_state - o));
  memcpy(head, &A, sizeof(A));
  memcpy(head + (l.off_step - o), step, (size_t)A.nA * sizeof(double));
  memcpy(head + (l.off_lo - o), g_lo, n * sizeof(double));
  memcpy(head + (l.off_hi - o), g_hi, n * sizeof(double));
  memcpy(head + (l.off_goals - o), goals, (size_t)A.n_ckt * (size_t)A.n_scalar * sizeof(SpiceyFitGoal));
  if (valid) memcpy(head + (l.off_valid - o), valid, (size_t)l.n_inst);
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The design kernel, enqueued on `st` behind a copy of `A` (HOST, from spicey_fit_design_judge), act and step into the design's
// head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_fit_design(int device, const SpiceyFitArgs &A, const int32_t *act, const double *step, void *d_work, hipStream_t st);
// The update kernel, one workgroup per circuit, behind a copy of `A` (HOST, from spicey_fit_update_judge) and of the HOST arrays
// into the update's head of d_work; the circuits' state behind it stays as the last update left it.  staged: an earlier launch
// on this workspace left step, g_lo, g_hi and goals there and they have not changed — only the record and valid go up.
hipError_t spicey_launch_fit_update(int device, const SpiceyFitArgs &A, const double *step, const double *g_lo, const double *g_hi, const SpiceyFitGoal *goals,
                                    const uint8_t *valid, void *d_work, hipStream_t st, bool staged = false);
#endif
