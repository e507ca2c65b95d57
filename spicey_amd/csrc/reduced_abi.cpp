// reduced_abi.cpp — the reduced runs of include/spicey_hip.h: one transient run into device buffers of the call's own and the
// reduction passes behind it (measure, fourier, timing, spectrum, power, values), through the positional entry points
// spicey_run_measure*, the struct entry point spicey_run_reduced, and the studies spicey_run_mc / spicey_run_sens /
// spicey_run_levels, which write the element values on the device first and reduce the passes' rows across the instances
// afterwards.  One driver (run_reduced) serves them all; a study is the hook it calls where the studies differ.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "tran_handle.h"
#include "fourier.h"
#include "fourier_exec.h"
#include "measure.h"
#include "measure_exec.h"
#include "power.h"
#include "values.h"
#include "spectrum.h"
#include "timing.h"
#include "timing_exec.h"
#include "tran_mc.h"
#include "tran_sens.h"

// One pass's list as the caller gave it: the requests, their count, the result pointer and (fourier, spectrum, values) the row
// length.  A call's lists are indexed by PASS_*; the values pass has its point table beside them.
struct PassList { const void *reqs; int32_t n; double *out; int32_t stride; };
// entry = the positional entry point's own pass, its last: that list may not be empty, the lists before it may, and there are
// none behind it.  entry = -1 (the struct entry points): every list may be empty but not all of them, and a pass runs iff its
// count is > 0.
struct RunLists { int entry; PassList l[N_PASS]; const SpiceyValPoint *pts; int64_t n_pts; };
static const int32_t fixed_row[N_PASS] = {8, 0, 8, 0, SPICEY_POWER_ROW, 0};  // doubles of a result row where the caller states none
static const int row_pass[SPICEY_TMC_N_PASS] = {PASS_MEASURE, PASS_TIMING, PASS_POWER};  // the passes whose rows a study's scalars read

// A study: what spicey_run_mc (the draw, the statistics across the samples) and spicey_run_sens / spicey_run_levels (the design, the
// sensitivities or the scalars alone) add to a reduced run, as far as they differ.  The driver owns the rest: the scratch value
// arrays and the workspace, the events, the placeholder rows, the instances' validity, the device results and the order of it all.
struct Study {
  const char *prefix = "", *no_valid = "";  // of the study's texts; what is missing when nothing can be reduced
  double SpiceyHandle::*ms = nullptr, SpiceyHandle::*design_ms = nullptr;  // the readouts of the reduction and of the draw or design
  bool results_null = false;       // a result buffer the call needs is missing
  bool need_nominal = false;       // reducible iff instance 0 is valid (else: iff any instance is)
  const void *some_out = nullptr;  // stands in for the call's result buffer in check_run_args
  // the results behind the run, in the order they go back: the caller's array (null: not wanted) and its bytes (0: none); set by judge
  struct Out { void *host; size_t bytes; } out[4] = {};
  // every refusal of the study's own arguments into h->err, on placeholder rows and buffers; work_bytes: its workspace
  virtual bool judge(SpiceyHandle *h, const SpiceyMcRows *rows, int64_t &work_bytes) = 0;
  // the draw or design from the handle's values into the scratch arrays, enqueued on st
  virtual hipError_t design(SpiceyHandle *h, double *oR, double *oC, double *oL, void *d_work, hipStream_t st) = 0;
  // the reduction over the passes' rows (valid: null when every instance is) into the device results d_out, as `out` numbers them
  virtual hipError_t launch(int device, const double *const *rows, const uint8_t *valid, void *const *d_out, void *d_work, hipStream_t st) = 0;
};

struct McStudy final : Study {
  const SpiceyTranMcReq *req = nullptr; const double *tol = nullptr, *icdf = nullptr;
  const SpiceyMcScalar *scalars = nullptr; int32_t n_scalar = 0;
  const double *lo = nullptr, *hi = nullptr, *probs = nullptr; int32_t n_prob = 0;
  double *stat = nullptr; int64_t *sample = nullptr; double *x = nullptr;
  SpiceyMcDrawArgs D{};
  SpiceyTmcArgs A{};
  bool judge(SpiceyHandle *h, const SpiceyMcRows *rows, int64_t &work_bytes) override {
    const SpiceyProg &P = h->hp.hdr;
    const int32_t ni = h->plan.n_inst;
    double dummy = 0.0, *some = &dummy;  // (any non-null pointer: the judges look at null-ness only)
    const int64_t draw_bytes = req ? spicey_mc_draw_bytes(P.nR + P.nC + P.nL, req->log2K) : 0;
    const int64_t red_bytes = spicey_tmc_reduce_bytes(ni, n_scalar, n_prob);
    work_bytes = std::max(draw_bytes, red_bytes);
    out[0] = {stat, (size_t)n_scalar * (size_t)(SPICEY_TMC_STAT_HEAD + 2 * n_prob) * sizeof(double)}, out[1] = {sample, (size_t)ni * 2 * sizeof(int64_t)};
    out[2] = {x, (size_t)ni * (size_t)n_scalar * sizeof(double)};
    return spicey_tmc_draw_judge(ni, P.nR, P.nC, P.nL, some, some, some, tol, icdf, req, some, some, some, true, draw_bytes, D, h->err) &&
           spicey_tmc_reduce_judge(ni, rows, scalars, n_scalar, lo, hi, probs, n_prob, true, red_bytes, A, h->err);
  }
  hipError_t design(SpiceyHandle *h, double *oR, double *oC, double *oL, void *d_work, hipStream_t st) override {
    D.R = h->d_R; D.C = h->d_C; D.L = h->d_L; D.oR = oR; D.oC = oC; D.oL = oL;
    return spicey_launch_tmc_draw(h->device, D, tol, icdf, d_work, st);
  }
  hipError_t launch(int device, const double *const *rows, const uint8_t *valid, void *const *d_out, void *d_work, hipStream_t st) override {
    for (int p = 0; p < SPICEY_TMC_N_PASS; p++) A.rows[p] = A.n_rows[p] > 0 ? rows[p] : nullptr;
    return spicey_launch_tmc_reduce(device, A, scalars, valid, lo, hi, probs, (double *)d_out[2], (double *)d_out[0], (int64_t *)d_out[1], d_work, st);
  }
};

struct SensStudy final : Study {
  int32_t mode = 0;  // the design the entry point takes; LEVELS: the scalars alone, no reduction across the instances
  const SpiceyTranSensReq *req = nullptr; const int32_t *act = nullptr; const double *step = nullptr; const int8_t *lvl = nullptr; const double *tol = nullptr;
  const SpiceyMcScalar *scalars = nullptr; int32_t n_scalar = 0;
  double *sens = nullptr; int8_t *sign = nullptr; double *bound = nullptr, *x = nullptr;
  SpiceyTsDesignArgs D{};
  SpiceyTmcArgs T{};
  SpiceyTsReduceArgs A{};
  std::vector<double> tol_act;
  bool judge(SpiceyHandle *h, const SpiceyMcRows *rows, int64_t &work_bytes) override {
    const SpiceyProg &P = h->hp.hdr;
    double dummy = 0.0, *some = &dummy;
    const int32_t ni = h->plan.n_inst, nE = P.nR + P.nC + P.nL, nA = req ? req->nA : 0;
    if (!spicey_ts_design_judge(ni, P.nR, P.nC, P.nL, some, some, some, req, mode, act, step, lvl, tol, some, some, some, true, INT64_MAX, D, h->err)) return false;
    if (mode == SPICEY_TS_LEVELS) {
      if (!spicey_ts_scalar_judge(ni, rows, scalars, n_scalar, true, T, h->err)) return false;
    } else {
      if (!tol) { h->err = "tran sens: null buffer"; return false; }
      if (const char *what = spicey_ts_judge_tol(tol, nE)) { h->err = std::string("tran sens: ") + what; return false; }
      tol_act.resize((size_t)nA);
      for (int32_t k = 0; k < nA; k++) tol_act[(size_t)k] = tol[act[k]];
      if (!spicey_ts_reduce_judge(ni, rows, scalars, n_scalar, step, tol_act.data(), nA, true, INT64_MAX, T, A, h->err)) return false;
      const size_t n_el = (size_t)n_scalar * (size_t)nA;
      out[0] = {sens, 2 * n_el * sizeof(double)}, out[1] = {sign, n_el}, out[2] = {bound, (size_t)n_scalar * SPICEY_TS_BOUND_ROW * sizeof(double)};
    }
    out[3] = {x, (size_t)ni * (size_t)n_scalar * sizeof(double)};
    work_bytes = spicey_ts_workspace_bytes(ni, n_scalar, nE, nA);
    return true;
  }
  hipError_t design(SpiceyHandle *h, double *oR, double *oC, double *oL, void *d_work, hipStream_t st) override {
    D.R = h->d_R; D.C = h->d_C; D.L = h->d_L; D.oR = oR; D.oC = oC; D.oL = oL;
    return spicey_launch_ts_design(h->device, D, act, step, lvl, tol, d_work, st);
  }
  hipError_t launch(int device, const double *const *rows, const uint8_t *valid, void *const *d_out, void *d_work, hipStream_t st) override {
    for (int p = 0; p < SPICEY_TMC_N_PASS; p++) T.rows[p] = T.n_rows[p] > 0 ? rows[p] : nullptr;
    if (mode == SPICEY_TS_LEVELS) return spicey_launch_tmc_scalars(device, T, scalars, valid, nullptr, nullptr, nullptr, (double *)d_out[3], d_work, st);
    return spicey_launch_ts_reduce(device, T, A, scalars, valid, step, tol_act.data(), (double *)d_out[3], (double *)d_out[0], (int8_t *)d_out[1], (double *)d_out[2], d_work, st);
  }
};

// What the entry points share: one transient run into device buffers of this call's own, the reductions on the handle's stream
// behind it, and only their results and `iters` on the way back.  study: null, or what a Monte Carlo, sensitivity or levels run
// adds — the run then reads scratch value arrays and its passes' rows stay on the device.
static int32_t run_reduced(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const RunLists &a, int32_t *iters,
                           Study *study = nullptr) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const PassList *l = a.l;
  if (study) {
    h->*study->ms = h->*study->design_ms = 0.0;
    const char *what = study->results_null ? "null buffer"
                       : l[PASS_FOURIER].n > 0 || l[PASS_SPECTRUM].n > 0 || l[PASS_VALUES].n > 0
                           ? "the fourier, spectrum and values lists are not reduced by this call (measure, timing and power are)" : nullptr;
    if (what) { forget_last_run(h); h->err = std::string(study->prefix) + what; return SPICEY_ERR_BAD_DESC; }
  }
  if (a.entry < 0) {
    int first_on = -1;
    for (int p = N_PASS - 1; p >= 0; p--) {
      if (l[p].n < 0) { forget_last_run(h); h->err = "reduced: every count must be >= 0"; return SPICEY_ERR_BAD_DESC; }
      if (l[p].n > 0) first_on = p;
    }
    if (first_on < 0) { forget_last_run(h); h->err = "reduced: every list is empty (at least one count must be > 0)"; return SPICEY_ERR_BAD_DESC; }
    // (a study leaves the passes' rows on the device: what it brings back is its own, and the lists' result pointers are not looked at)
    if (const int32_t rc0 = check_run_args(h, steps, study ? study->some_out : l[first_on].out, src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
    for (int p = 0; p < N_PASS && !study; p++)
      if (l[p].n > 0 && !l[p].out) { h->err = "reduced: a result pointer is null where its count is > 0"; return SPICEY_ERR_BAD_DESC; }
  } else if (const int32_t rc0 = check_run_args(h, steps, l[a.entry].out, src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
  // (a positional entry point's own refusal: a list before its own with a negative count, or a count > 0 and no result pointer)
  static const char *const entry_text[N_PASS] = {
      nullptr, "fourier: n_req must be >= 0, and meas not null when n_req > 0", "timing: n_req and n_four must be >= 0, and meas / four not null when their count is > 0",
      "spectrum: n_req, n_four and n_timing must be >= 0, and meas / four / timing not null when their count is > 0",
      "power: n_req, n_four, n_timing and n_spec must be >= 0, and meas / four / timing / spec not null when their count is > 0", nullptr};
  for (int p = 0; p < a.entry; p++)
    if (l[p].n < 0 || (l[p].n > 0 && !l[p].out)) { h->err = entry_text[a.entry]; return SPICEY_ERR_BAD_DESC; }
  // (a pass runs if it is the entry point's own, or an earlier one whose list is not empty)
  bool on[N_PASS];
  for (int p = 0; p < N_PASS; p++) on[p] = a.entry < 0 ? l[p].n > 0 : p == a.entry || (p < a.entry && l[p].n != 0);
  const SpiceyProg &P = h->hp.hdr;
  const int32_t ni = h->plan.n_inst;
  const int64_t np = steps + 1;
  const int32_t n_req = l[PASS_MEASURE].n, n_tim = l[PASS_TIMING].n, n_power = l[PASS_POWER].n;
  // (a refused request list runs nothing; the buffers are this call's own)
  const int64_t work_bytes = on[PASS_MEASURE] ? spicey_meas_workspace_bytes(ni, np, n_req) : 0;
  std::vector<SpiceyMeasDevReq> table;
  if (on[PASS_MEASURE])
    if (const int32_t rc0 = spicey_judge_measure("measure", spicey_meas_plan, spicey_meas_workspace_bytes, ni, np, true, P.nOut, true, P.nCur,
                                                 (const SpiceyMeasReq *)l[PASS_MEASURE].reqs, n_req, true, work_bytes, table, h->err); rc0 != SPICEY_OK)
      return rc0;
  SpiceyFourPlan fplan;
  if (on[PASS_FOURIER] && !spicey_four_judge(ni, np, dt, true, P.nOut, true, P.nCur, (const SpiceyFourReq *)l[PASS_FOURIER].reqs, l[PASS_FOURIER].n, true,
                                             l[PASS_FOURIER].stride, INT64_MAX, fplan, h->err))
    return SPICEY_ERR_BAD_DESC;
  SpiceyTimPlan tplan;
  if (on[PASS_TIMING] && !spicey_tim_judge(ni, np, dt, true, P.nOut, true, P.nCur, (const SpiceyTimingReq *)l[PASS_TIMING].reqs, n_tim, true, INT64_MAX, tplan, h->err))
    return SPICEY_ERR_BAD_DESC;
  SpiceySpecPlan splan;
  if (on[PASS_SPECTRUM] && !spicey_spec_judge(ni, np, dt, true, P.nOut, true, P.nCur, (const SpiceySpecReq *)l[PASS_SPECTRUM].reqs, l[PASS_SPECTRUM].n, true,
                                              l[PASS_SPECTRUM].stride, INT64_MAX, splan, h->err))
    return SPICEY_ERR_BAD_DESC;
  std::vector<SpiceyPowerDevReq> ptable;
  if (on[PASS_POWER] && !spicey_power_judge(ni, np, dt, true, P.nOut, true, P.nCur, (const SpiceyPowerReq *)l[PASS_POWER].reqs, n_power, true, INT64_MAX, ptable, h->err))
    return SPICEY_ERR_BAD_DESC;
  SpiceyValPlan vplan;
  if (on[PASS_VALUES] && !spicey_val_judge(ni, np, dt, true, P.nOut, true, P.nCur, (const SpiceyValReq *)l[PASS_VALUES].reqs, l[PASS_VALUES].n, a.pts, a.n_pts,
                                           on[PASS_TIMING], n_tim, true, l[PASS_VALUES].stride, INT64_MAX, vplan, h->err))
    return SPICEY_ERR_BAD_DESC;
  // (the study's request, arrays and programs, judged on placeholder rows: the scratch arrays and the passes' rows are bound below)
  int64_t study_work_bytes = 0;
  if (study) {
    double dummy = 0.0;
    SpiceyMcRows jr[SPICEY_TMC_N_PASS];
    for (int p = 0; p < SPICEY_TMC_N_PASS; p++) jr[p] = {on[row_pass[p]] ? &dummy : nullptr, on[row_pass[p]] ? l[row_pass[p]].n : 0, fixed_row[row_pass[p]]};
    if (!study->judge(h, jr, study_work_bytes)) return SPICEY_ERR_BAD_DESC;
  }
  const auto names_a_current = [](const auto &list) { return std::any_of(list.begin(), list.end(), [](const auto &q) { return q.signal == 1; }); };
  const bool need_i = names_a_current(table) || names_a_current(fplan.table) || names_a_current(tplan.edges) || names_a_current(splan.table) ||
                      std::any_of(ptable.begin(), ptable.end(), [](const SpiceyPowerDevReq &q) { return q.a_signal == 1 || q.b_signal == 1; }) ||
                      names_a_current(vplan.traces) || std::any_of(vplan.points.begin(), vplan.points.end(), [](const SpiceyValDevPts &q) {
                        return q.signal == 1 || (q.kind == SPICEY_VAL_FIND && q.x_signal == 1);
                      });
  if (const int32_t rc0 = check_structure(h); rc0 != SPICEY_OK) return rc0;
  HIPCHK(h, hipSetDevice(h->device));
  static const char *const entry_name[N_PASS] = {"spicey_run_measure", "spicey_run_measure_fourier", "spicey_run_measure_timing", "spicey_run_measure_spectrum",
                                                 "spicey_run_measure_power", "spicey_run_reduced"};
  Roctx range_run(entry_name[a.entry < 0 ? N_PASS - 1 : a.entry]);
  HostRun r;
  hipStream_t st = h->q.stream;
  // The pass table: what the blocks below do per pass.  A further pass is one more entry here (and its judge above).
  struct Pass {
    size_t work_bytes;   // bytes of the workspace
    const char *failed;  // prefix of a launch error's text
    std::function<hipError_t(double *d_out, void *d_work)> launch;
    size_t n_out;        // doubles of the result
    DevBuf<double> d_out;
    DevBuf<uint8_t> d_work;
  };
  const double *d_timing_rows = nullptr;  // (the timing pass's device rows, once they are allocated: the values pass reads them)
  Pass pass[N_PASS] = {
      {(size_t)work_bytes, "spicey_launch_measure: ", [&](double *d_out, void *d_work) {
         return spicey_launch_measure(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, table.data(), n_req, d_out, d_work, st);
       }},
      {(size_t)fplan.workspace_bytes(ni), "spicey_launch_fourier: ", [&](double *d_out, void *d_work) {
         return spicey_launch_fourier(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, fplan, d_out, l[PASS_FOURIER].stride, d_work, st);
       }},
      {(size_t)tplan.workspace_bytes(ni, np), "spicey_launch_timing: ", [&](double *d_out, void *d_work) {
         return spicey_launch_timing(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, tplan, d_out, d_work, st);
       }},
      {(size_t)splan.workspace_bytes(), "spicey_launch_spectrum: ", [&](double *d_out, void *d_work) {
         return spicey_launch_spectrum(h->device, ni, np, r.d_v, P.nOut, r.d_i, P.nCur, splan, d_out, l[PASS_SPECTRUM].stride, d_work, st);
       }},
      {on[PASS_POWER] ? (size_t)spicey_pow_workspace_bytes(ni, np, n_power) : 0, "spicey_launch_power: ", [&](double *d_out, void *d_work) {
         return spicey_launch_power(h->device, ni, np, r.d_v, P.nOut, r.d_i, P.nCur, ptable.data(), n_power, d_out, d_work, st);
       }},
      {on[PASS_VALUES] ? (size_t)vplan.workspace_bytes(ni) : 0, "spicey_launch_values: ", [&](double *d_out, void *d_work) {
         return spicey_launch_values(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, vplan, a.pts, d_timing_rows, n_tim, d_out, l[PASS_VALUES].stride, d_work, st);
       }},
  };
  for (int p = 0; p < N_PASS; p++)
    if (on[p]) HIPCHK(h, h->q.want_pass_events(p));
  // (no current request: the run records no currents)
  if (const int32_t rc0 = r.stage(h, steps, src_table, src_per_inst, need_i, iters != nullptr); rc0 != SPICEY_OK) return rc0;
  for (int p = 0; p < N_PASS; p++) {
    if (!on[p]) continue;
    pass[p].n_out = (size_t)ni * (size_t)l[p].n * (size_t)(fixed_row[p] ? fixed_row[p] : l[p].stride);
    HIPCHK(h, pass[p].d_out.alloc(pass[p].n_out));
    HIPCHK(h, pass[p].d_work.alloc(pass[p].work_bytes));
  }
  if (on[PASS_TIMING]) d_timing_rows = pass[PASS_TIMING].d_out;
  for (double &ms : h->last_pass_ms) ms = 0.0;
  // (a study: the draw or design into scratch value arrays of this call's own, which the transient then reads; they live until
  // the call returns, so a launch that spicey_sync repeats reads them again)
  DevBuf<double> d_sR, d_sC, d_sL;
  DevBuf<uint8_t> d_study_work;
  EventPair ev_design, ev_red;
  const double *study_vals[3] = {nullptr, nullptr, nullptr};
  if (study) {
    HIPCHK(h, d_sR.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nR)));
    HIPCHK(h, d_sC.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nC)));
    HIPCHK(h, d_sL.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nL)));
    HIPCHK(h, d_study_work.alloc((size_t)study_work_bytes));
    HIPCHK(h, ev_design.create());
    HIPCHK(h, ev_red.create());
    HIPCHK(h, hipEventRecord(ev_design.a, st));
    HIPCHK(h, study->design(h, d_sR, d_sC, d_sL, d_study_work, st));
    HIPCHK(h, hipEventRecord(ev_design.b, st));
    study_vals[0] = d_sR; study_vals[1] = d_sC; study_vals[2] = d_sL;
  }
  int32_t rc = run_device_src(h, steps, dt, r.d_src, src_per_inst, r.d_v, r.d_i, r.d_it, st, study ? study_vals : nullptr);
  if (rc != SPICEY_OK) return rc;
  const char *failed = "";
  auto reduce = [&]() {
    hipError_t e = hipSuccess;
    for (int p = 0; p < N_PASS && e == hipSuccess; p++) {
      if (!on[p]) continue;
      failed = pass[p].failed;
      e = hipEventRecord(h->q.pass_ev[p][0], st);
      if (e == hipSuccess) e = pass[p].launch(pass[p].d_out, pass[p].d_work);
      if (e == hipSuccess) e = hipEventRecord(h->q.pass_ev[p][1], st);
    }
    return e;
  };
  const int retries = h->group_retries;
  hipError_t e = reduce();
  rc = spicey_sync(h);  // (the stream's end: the transient's status, with the reductions behind it; also before the buffers go)
  // (group mode with group_retry: spicey_sync repeated the transient behind the reductions, so the reductions run again)
  if (e == hipSuccess && h->group_retries != retries && rc == SPICEY_OK && (e = reduce()) == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { h->err = std::string(failed) + hipGetErrorString(e); return SPICEY_ERR_HIP; }
  if (rc != SPICEY_OK && rc != SPICEY_ERR_SINGULAR) return rc;
  for (int p = 0; p < N_PASS; p++)
    if (on[p]) StreamTimers::elapsed(h->q.pass_ev[p][0], h->q.pass_ev[p][1], &h->last_pass_ms[p]);
  if (study) {
    StreamTimers::elapsed(ev_design.a, ev_design.b, &(h->*study->design_ms));
    std::vector<int32_t> ist((size_t)ni);
    std::vector<uint8_t> valid((size_t)ni);
    spicey_last_inst_status(h, ist.data());
    int32_t n_valid = 0;
    for (int32_t s = 0; s < ni; s++) n_valid += valid[(size_t)s] = ist[(size_t)s] == 0;
    // (a sample or instance is valid iff it finished; with nothing to reduce the outputs stay as they are)
    if (study->need_nominal ? valid[0] != 0 : n_valid > 0) {
      // (the study's record was judged before anything ran, on placeholders: the passes' rows take their place)
      const double *rows[SPICEY_TMC_N_PASS];
      for (int p = 0; p < SPICEY_TMC_N_PASS; p++) rows[p] = pass[row_pass[p]].d_out;
      DevBuf<uint8_t> d_res[4];
      void *d_out[4];
      for (int k = 0; k < 4; k++) {
        if (study->out[k].bytes) HIPCHK(h, d_res[k].alloc(study->out[k].bytes));
        d_out[k] = d_res[k];
      }
      HIPCHK(h, hipEventRecord(ev_red.a, st));
      HIPCHK(h, study->launch(h->device, rows, n_valid == ni ? nullptr : valid.data(), d_out, d_study_work, st));
      HIPCHK(h, hipEventRecord(ev_red.b, st));
      for (int k = 0; k < 4; k++)
        if (study->out[k].host && study->out[k].bytes) HIPCHK(h, hipMemcpyAsync(study->out[k].host, d_out[k], study->out[k].bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      StreamTimers::elapsed(ev_red.a, ev_red.b, &(h->*study->ms));
    } else if (rc == SPICEY_OK) {
      h->err = std::string(study->prefix) + study->no_valid;
      rc = SPICEY_ERR_SINGULAR;
    } else h->err += std::string(" (") + study->prefix + study->no_valid + ", nothing reduced)";
  } else {
    Roctx range_copy("spicey_run_measure:results");
    for (int p = 0; p < N_PASS; p++)
      if (on[p]) HIPCHK(h, hipMemcpy(l[p].out, pass[p].d_out, pass[p].n_out * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (const int32_t rc0 = r.copy_out(h, nullptr, nullptr, iters); rc0 != SPICEY_OK) return rc0;
  return rc;
}

// The struct entry points: the header's refusals under the entry point's own texts ("reduced: struct_bytes ...", "tran mc:
// lists.struct_bytes ..."), every list from the struct — a study takes no result pointers, its rows stay on the device — the driver.
static int32_t run_struct(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *s, int32_t *iters,
                          Study *study = nullptr) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const char *what = !s ? "lists must not be null"
                     : s->struct_bytes < (int64_t)sizeof(SpiceyReducedLists) ? "struct_bytes is smaller than sizeof(SpiceyReducedLists)"
                     : s->reserved != 0 ? "reserved must be 0" : nullptr;
  if (what) { forget_last_run(h); h->err = std::string(study ? study->prefix : "reduced: ") + (s && study ? "lists." : "") + what; return SPICEY_ERR_BAD_DESC; }
  RunLists a{-1, {{s->reqs, s->n_req, s->meas, 0}, {s->freqs, s->n_four, s->four, s->four_stride}, {s->treqs, s->n_timing, s->timing, 0},
                  {s->sreqs, s->n_spec, s->spec, s->spec_stride}, {s->preqs, s->n_power, s->power, 0}, {s->vreqs, s->n_values, s->values, s->values_stride}},
             s->pts, s->n_pts};
  for (PassList &l : a.l)
    if (study) l.out = nullptr;
  return run_reduced(h, steps, dt, src_table, src_per_inst, a, iters, study);
}

extern "C" int32_t spicey_run_mc(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                 const SpiceyTranMcReq *req, const double *tol, const double *icdf, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                 const double *lo, const double *hi, const double *probs, int32_t n_prob, double *stat, int64_t *sample, double *x,
                                 int32_t *iters) {
  McStudy s;
  s.prefix = "tran mc: "; s.no_valid = "no valid sample"; s.ms = &SpiceyHandle::last_tran_mc_ms; s.design_ms = &SpiceyHandle::last_tran_mc_draw_ms;
  s.results_null = !stat || !sample; s.some_out = stat;
  s.req = req; s.tol = tol; s.icdf = icdf; s.scalars = scalars; s.n_scalar = n_scalar; s.lo = lo; s.hi = hi; s.probs = probs; s.n_prob = n_prob;
  s.stat = stat; s.sample = sample; s.x = x;
  return run_struct(h, steps, dt, src_table, src_per_inst, l, iters, &s);
}

// (s: the call's own arguments set)
static int32_t run_tran_sens(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l, int32_t *iters,
                             SensStudy &s) {
  const bool levels = s.mode == SPICEY_TS_LEVELS;  // a sensitivity needs the nominal instance, a levels run any instance
  s.prefix = "tran sens: "; s.no_valid = levels ? "no valid instance" : "the nominal instance is not valid";
  s.ms = &SpiceyHandle::last_tran_sens_ms; s.design_ms = &SpiceyHandle::last_tran_sens_design_ms;
  s.results_null = levels ? !s.x : (!s.sens || !s.sign || !s.bound); s.need_nominal = !levels; s.some_out = levels ? s.x : s.bound;
  return run_struct(h, steps, dt, src_table, src_per_inst, l, iters, &s);
}

extern "C" int32_t spicey_run_sens(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                   const SpiceyTranSensReq *req, const int32_t *act, const double *step, const double *tol, const SpiceyMcScalar *scalars,
                                   int32_t n_scalar, double *sens, int8_t *sign, double *bound, double *x, int32_t *iters) {
  SensStudy s;
  s.mode = SPICEY_TS_ONE_AT_A_TIME; s.req = req; s.act = act; s.step = step; s.tol = tol; s.scalars = scalars; s.n_scalar = n_scalar;
  s.sens = sens; s.sign = sign; s.bound = bound; s.x = x;
  return run_tran_sens(h, steps, dt, src_table, src_per_inst, l, iters, s);
}

extern "C" int32_t spicey_run_levels(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                     const SpiceyTranSensReq *req, const int8_t *lvl, const double *tol, const SpiceyMcScalar *scalars, int32_t n_scalar, double *x,
                                     int32_t *iters) {
  SensStudy s;
  s.mode = SPICEY_TS_LEVELS; s.req = req; s.lvl = lvl; s.tol = tol; s.scalars = scalars; s.n_scalar = n_scalar; s.x = x;
  return run_tran_sens(h, steps, dt, src_table, src_per_inst, l, iters, s);
}

extern "C" int32_t spicey_run_reduced(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *l,
                                      int32_t *iters) {
  return run_struct(h, steps, dt, src_table, src_per_inst, l, iters);
}

// The positional entry points: the lists up to the entry point's own.
extern "C" int32_t spicey_run_measure(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                      int32_t n_req, double *meas, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst, {0, {{reqs, n_req, meas}}}, iters);
}

extern "C" int32_t spicey_run_measure_fourier(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                              int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                              int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst, {1, {{reqs, n_req, meas}, {freqs, n_four, four, four_stride}}}, iters);
}

extern "C" int32_t spicey_run_measure_timing(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                             int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                             const SpiceyTimingReq *treqs, int32_t n_timing, double *timing, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst, {2, {{reqs, n_req, meas}, {freqs, n_four, four, four_stride}, {treqs, n_timing, timing}}}, iters);
}

extern "C" int32_t spicey_run_measure_spectrum(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                               int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                               const SpiceyTimingReq *treqs, int32_t n_timing, double *timing, const SpiceySpecReq *sreqs, int32_t n_spec, double *spec,
                                               int32_t spec_stride, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst,
                     {3, {{reqs, n_req, meas}, {freqs, n_four, four, four_stride}, {treqs, n_timing, timing}, {sreqs, n_spec, spec, spec_stride}}}, iters);
}

extern "C" int32_t spicey_run_measure_power(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyMeasReq *reqs,
                                            int32_t n_req, double *meas, const SpiceyFourReq *freqs, int32_t n_four, double *four, int32_t four_stride,
                                            const SpiceyTimingReq *treqs, int32_t n_timing, double *timing, const SpiceySpecReq *sreqs, int32_t n_spec, double *spec,
                                            int32_t spec_stride, const SpiceyPowerReq *preqs, int32_t n_power, double *power, int32_t *iters) {
  return run_reduced(h, steps, dt, src_table, src_per_inst,
                     {4, {{reqs, n_req, meas}, {freqs, n_four, four, four_stride}, {treqs, n_timing, timing}, {sreqs, n_spec, spec, spec_stride}, {preqs, n_power, power}}},
                     iters);
}

extern "C" double spicey_last_measure_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_MEASURE] : 0.0; }
extern "C" double spicey_last_fourier_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_FOURIER] : 0.0; }
extern "C" double spicey_last_timing_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_TIMING] : 0.0; }
extern "C" double spicey_last_spectrum_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_SPECTRUM] : 0.0; }
extern "C" double spicey_last_power_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_POWER] : 0.0; }
extern "C" double spicey_last_values_ms(SpiceyHandle *h) { return h ? h->last_pass_ms[PASS_VALUES] : 0.0; }
extern "C" double spicey_last_tran_mc_ms(SpiceyHandle *h) { return h ? h->last_tran_mc_ms : 0.0; }
extern "C" double spicey_last_tran_mc_draw_ms(SpiceyHandle *h) { return h ? h->last_tran_mc_draw_ms : 0.0; }
extern "C" double spicey_last_tran_sens_ms(SpiceyHandle *h) { return h ? h->last_tran_sens_ms : 0.0; }
extern "C" double spicey_last_tran_sens_design_ms(SpiceyHandle *h) { return h ? h->last_tran_sens_design_ms : 0.0; }
