// fit_abi.cpp — spicey_run_fit of include/spicey_hip.h: the damped least-squares loop on a handle.  The source table, the
// outputs, the passes' rows and workspaces are staged once; per iteration the handle's state at entry is restored, the design
// writes scratch value arrays, ONE transient bound to them runs exactly as under spicey_run_sens, the measure / timing / power
// passes leave their rows on the device, the scalar kernel of tran_mc.hip turns them into x and the update of fit.hip moves the
// gains; only the [n_ckt][8] rows and the done flags come back.  The transient is synchronised before the scalars are enqueued:
// a group-mode launch that spicey_sync repeats is followed by its passes again, and the update knows the instances' statuses.
// A driver of its own beside reduced_abi.cpp's: that one runs its section once and brings a study's results back, this one
// repeats the section and keeps everything on the device; they share HostRun, the judges and the pass launchers.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <vector>

#include "tran_handle.h"
#include "fit.h"
#include "measure.h"
#include "measure_exec.h"
#include "power.h"
#include "timing.h"
#include "timing_exec.h"
#include "tran_mc.h"

namespace {
int32_t refuse(SpiceyHandle *h, const std::string &what) {
  forget_last_run(h);
  h->err = what.rfind("fit: ", 0) == 0 ? what : "fit: " + what;
  return SPICEY_ERR_BAD_DESC;
}
}  // namespace

extern "C" int32_t spicey_run_fit(SpiceyHandle *h, int64_t steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyReducedLists *s,
                                  const SpiceyFitReq *req, const int32_t *act, const double *step, const double *g_lo, const double *g_hi, const double *g0,
                                  const SpiceyFitGoal *goals, const SpiceyMcScalar *scalars, int32_t n_scalar, double *g, double *F, double *history,
                                  int32_t *n_iter, int32_t *status, double *x, int32_t *iters) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  h->last_fit_ms = h->last_fit_tran_ms = 0.0;
  const SpiceyProg &P = h->hp.hdr;
  const int32_t ni = h->plan.n_inst;
  const int64_t np = steps + 1;
  // ---- every refusal, before the device is touched
  if (const char *what = spicey_fit_judge_req(req, true)) return refuse(h, what);
  if (!s) return refuse(h, "lists must not be null");
  if (s->struct_bytes < (int64_t)sizeof(SpiceyReducedLists)) return refuse(h, "lists.struct_bytes is smaller than sizeof(SpiceyReducedLists)");
  if (s->reserved != 0) return refuse(h, "lists.reserved must be 0");
  if (s->n_four > 0 || s->n_spec > 0 || s->n_values > 0)
    return refuse(h, "the fourier, spectrum and values lists are not reduced by this call (measure, timing and power are)");
  if (s->n_req < 0 || s->n_four < 0 || s->n_timing < 0 || s->n_spec < 0 || s->n_power < 0 || s->n_values < 0) return refuse(h, "every count must be >= 0");
  if (s->n_req + s->n_timing + s->n_power == 0) return refuse(h, "every list is empty (at least one count must be > 0)");
  if (!g0 || !g || !F || !history || !n_iter || !status) return refuse(h, "null buffer");
  const int32_t n_ckt = req->n_ckt, nA = req->nA, W = 1 + 2 * nA;
  if ((int64_t)ni != (int64_t)n_ckt * W) {
    char buf[160];
    snprintf(buf, sizeof(buf), "the handle has %d instances, n_ckt W = %lld are needed (W = 1 + 2 nA = %d)", ni, (long long)n_ckt * W, W);
    return refuse(h, buf);
  }
  double dummy = 0.0, *some = &dummy;  // (any non-null pointer: the judges look at null-ness only)
  int32_t idummy = 0;
  SpiceyFitArgs D, U;
  std::string err;
  if (!spicey_fit_design_judge(P.nR, P.nC, P.nL, some, some, some, req, act, step, some, some, some, some, true, INT64_MAX, D, err)) return refuse(h, err);
  if (!spicey_fit_update_judge(req, n_scalar, 1, step, g_lo, g_hi, goals, some, some, some, &idummy, true, INT64_MAX, U, err)) return refuse(h, err);
  for (int64_t i = 0; i < (int64_t)n_ckt * nA; i++)
    if (!std::isfinite(g0[i]) || !(g0[i] > 0.0)) return refuse(h, "a starting gain must be finite and > 0");
  const int32_t n_req = s->n_req, n_tim = s->n_timing, n_pow = s->n_power;
  std::vector<SpiceyMeasDevReq> table;
  if (n_req) {
    if (const int32_t rc0 = spicey_judge_measure("measure", spicey_meas_plan, spicey_meas_workspace_bytes, ni, np, true, P.nOut, true, P.nCur, s->reqs, n_req, true,
                                                 spicey_meas_workspace_bytes(ni, np, n_req), table, h->err); rc0 != SPICEY_OK) {
      forget_last_run(h);
      return rc0;
    }
  }
  SpiceyTimPlan tplan;
  if (n_tim && !spicey_tim_judge(ni, np, dt, true, P.nOut, true, P.nCur, s->treqs, n_tim, true, INT64_MAX, tplan, h->err)) { forget_last_run(h); return SPICEY_ERR_BAD_DESC; }
  std::vector<SpiceyPowerDevReq> ptable;
  if (n_pow && !spicey_power_judge(ni, np, dt, true, P.nOut, true, P.nCur, s->preqs, n_pow, true, INT64_MAX, ptable, h->err)) { forget_last_run(h); return SPICEY_ERR_BAD_DESC; }
  const int32_t pass_n[SPICEY_TMC_N_PASS] = {n_req, n_tim, n_pow}, pass_row[SPICEY_TMC_N_PASS] = {8, 8, SPICEY_POWER_ROW};
  SpiceyMcRows jr[SPICEY_TMC_N_PASS];
  for (int p = 0; p < SPICEY_TMC_N_PASS; p++) jr[p] = {pass_n[p] ? some : nullptr, pass_n[p], pass_row[p]};
  SpiceyTmcArgs T;
  if (!spicey_tmc_reduce_judge(ni, jr, scalars, n_scalar, nullptr, nullptr, nullptr, 0, true, INT64_MAX, T, err)) return refuse(h, err.substr(err.rfind("tran mc: ", 0) == 0 ? 9 : 0));
  if (const int32_t rc0 = check_run_args(h, steps, g, src_table, src_per_inst); rc0 != SPICEY_OK) return rc0;
  const auto names_a_current = [](const auto &list) { return std::any_of(list.begin(), list.end(), [](const auto &q) { return q.signal == 1; }); };
  const bool need_i = names_a_current(table) || names_a_current(tplan.edges) ||
                      std::any_of(ptable.begin(), ptable.end(), [](const SpiceyPowerDevReq &q) { return q.a_signal == 1 || q.b_signal == 1; });
  for (int32_t c = 0; c < n_ckt; c++) { n_iter[c] = 0; status[c] = 1; F[c] = INFINITY; }
  memcpy(g, g0, (size_t)n_ckt * nA * sizeof(double));
  if (check_structure(h) == SPICEY_ERR_SINGULAR) {  // (every nominal run would fail in its first solve: as spicey_run_pss, a status per circuit)
    for (int32_t c = 0; c < n_ckt; c++) status[c] = 2;
    return SPICEY_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) {  // (a run still in flight: its end state is the state at entry)
    const int32_t rc0 = spicey_sync(h);
    forget_last_run(h);
    if (rc0 != SPICEY_OK && rc0 != SPICEY_ERR_SINGULAR) return rc0;
  }
  Roctx range_run("spicey_run_fit");
  hipStream_t st = h->q.stream;
  // ---- staged once
  const StatePtrs S = h->state.ptrs();
  const size_t st_n[4] = {(size_t)ni * P.nC * sizeof(double), (size_t)ni * P.nL * sizeof(double), (size_t)ni * P.nD * sizeof(double), (size_t)ni * P.nS * sizeof(int32_t)};
  void *const st_live[4] = {S.Cv, S.Li, S.Dv, S.Son};
  DevBuf<uint8_t> d_entry[4];
  for (int k = 0; k < 4; k++)
    if (st_n[k]) {
      HIPCHK(h, d_entry[k].alloc(st_n[k]));
      HIPCHK(h, hipMemcpyAsync(d_entry[k], st_live[k], st_n[k], hipMemcpyDeviceToDevice, st));
    }
  auto restore = [&]() {
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; k++)
      if (st_n[k]) e = hipMemcpyAsync(st_live[k], d_entry[k], st_n[k], hipMemcpyDeviceToDevice, st);
    return e;
  };
  // (whatever ends the call from here on, an error included: the handle's state is the state at entry)
  struct AtExit {
    decltype(restore) &f; hipStream_t st; bool armed;
    ~AtExit() { if (armed && f() == hipSuccess) (void)hipStreamSynchronize(st); }
  } at_exit{restore, st, true};
  HostRun r;
  if (const int32_t rc0 = r.stage(h, steps, src_table, src_per_inst, need_i, iters != nullptr); rc0 != SPICEY_OK) return rc0;
  DevBuf<double> d_sR, d_sC, d_sL, d_g, d_x, d_rows, d_pass[SPICEY_TMC_N_PASS];
  DevBuf<int32_t> d_done;
  DevBuf<uint8_t> d_work, d_tmc_work, d_pass_work[SPICEY_TMC_N_PASS];
  const int64_t work_bytes = spicey_fit_bytes(n_ckt, nA, n_scalar);
  const size_t pass_work[SPICEY_TMC_N_PASS] = {n_req ? (size_t)spicey_meas_workspace_bytes(ni, np, n_req) : 0, n_tim ? (size_t)tplan.workspace_bytes(ni, np) : 0,
                                               n_pow ? (size_t)spicey_pow_workspace_bytes(ni, np, n_pow) : 0};
  HIPCHK(h, d_sR.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nR)));
  HIPCHK(h, d_sC.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nC)));
  HIPCHK(h, d_sL.alloc(std::max<size_t>(1, (size_t)ni * (size_t)P.nL)));
  HIPCHK(h, d_g.alloc((size_t)n_ckt * nA));
  HIPCHK(h, d_x.alloc((size_t)ni * n_scalar));
  HIPCHK(h, d_rows.alloc((size_t)n_ckt * SPICEY_FIT_ROW));
  HIPCHK(h, d_done.alloc((size_t)n_ckt));
  HIPCHK(h, d_work.alloc((size_t)work_bytes));
  HIPCHK(h, d_tmc_work.alloc((size_t)spicey_tmc_reduce_bytes(ni, n_scalar, 0)));
  for (int p = 0; p < SPICEY_TMC_N_PASS; p++)
    if (pass_n[p]) {
      HIPCHK(h, d_pass[p].alloc((size_t)ni * pass_n[p] * pass_row[p]));
      HIPCHK(h, d_pass_work[p].alloc(std::max<size_t>(1, pass_work[p])));
    }
  HIPCHK(h, hipMemsetAsync(d_work, 0, (size_t)work_bytes, st));
  HIPCHK(h, hipMemsetAsync(d_rows, 0, (size_t)n_ckt * SPICEY_FIT_ROW * sizeof(double), st));
  HIPCHK(h, hipMemsetAsync(d_done, 0, (size_t)n_ckt * sizeof(int32_t), st));
  HIPCHK(h, hipMemcpyAsync(d_g, g0, (size_t)n_ckt * nA * sizeof(double), hipMemcpyHostToDevice, st));
  D.R = h->d_R; D.C = h->d_C; D.L = h->d_L; D.oR = d_sR; D.oC = d_sC; D.oL = d_sL; D.g = d_g;
  U.g = d_g; U.x = d_x; U.rows = d_rows; U.done = d_done;
  for (int p = 0; p < SPICEY_TMC_N_PASS; p++) T.rows[p] = pass_n[p] ? (const double *)d_pass[p] : nullptr;
  const double *vals[3] = {d_sR, d_sC, d_sL};
  const char *failed = "";
  auto reduce = [&]() {
    hipError_t e = hipSuccess;
    if (n_req) { failed = "spicey_launch_measure: "; e = spicey_launch_measure(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, table.data(), n_req, d_pass[0], d_pass_work[0], st); }
    if (n_tim && e == hipSuccess) { failed = "spicey_launch_timing: "; e = spicey_launch_timing(h->device, ni, np, dt, r.d_v, P.nOut, r.d_i, P.nCur, tplan, d_pass[1], d_pass_work[1], st); }
    if (n_pow && e == hipSuccess) { failed = "spicey_launch_power: "; e = spicey_launch_power(h->device, ni, np, r.d_v, P.nOut, r.d_i, P.nCur, ptable.data(), n_pow, d_pass[2], d_pass_work[2], st); }
    return e;
  };
  EventPair ev_design, ev_update;
  HIPCHK(h, ev_design.create());
  HIPCHK(h, ev_update.create());
  std::vector<int32_t> done((size_t)n_ckt, 0), ist((size_t)ni, 0);
  std::vector<uint8_t> valid((size_t)ni, 1);
  std::vector<double> x_nom(x ? (size_t)n_ckt * n_scalar : 0);
  std::string run_err;
  int32_t rc = SPICEY_OK;
  for (int32_t it = 0; it < req->max_iter; it++) {
    double *row_it = history + (size_t)it * n_ckt * SPICEY_FIT_ROW;
    HIPCHK(h, restore());
    HIPCHK(h, hipEventRecord(ev_design.a, st));
    HIPCHK(h, spicey_launch_fit_design(h->device, D, act, step, d_work, st));
    HIPCHK(h, hipEventRecord(ev_design.b, st));
    rc = run_device_src(h, steps, dt, r.d_src, src_per_inst, r.d_v, r.d_i, r.d_it, st, vals);
    if (rc != SPICEY_OK) return rc;
    const int retries = h->group_retries;
    hipError_t e = reduce();
    rc = spicey_sync(h);  // (the transient's status, with the passes behind it)
    // (group mode with group_retry: spicey_sync repeated the transient behind the passes, so the passes run again)
    if (e == hipSuccess && h->group_retries != retries && rc == SPICEY_OK) e = reduce();
    if (e != hipSuccess) { h->err = std::string(failed) + hipGetErrorString(e); return SPICEY_ERR_HIP; }
    if (rc != SPICEY_OK && rc != SPICEY_ERR_SINGULAR) return rc;
    if (rc == SPICEY_ERR_SINGULAR && run_err.empty()) run_err = h->err;
    const bool any_bad = spicey_last_inst_status(h, ist.data()) > 0;
    for (int32_t i = 0; i < ni; i++) valid[(size_t)i] = ist[(size_t)i] == 0;
    const uint8_t *va = any_bad ? valid.data() : nullptr;
    HIPCHK(h, spicey_launch_tmc_scalars(h->device, T, scalars, va, nullptr, nullptr, nullptr, d_x, d_tmc_work, st));
    HIPCHK(h, hipEventRecord(ev_update.a, st));
    U.first = it == 0;
    HIPCHK(h, spicey_launch_fit_update(h->device, U, step, g_lo, g_hi, goals, va, d_work, st, it > 0));  // (the head's arrays go up once)
    HIPCHK(h, hipEventRecord(ev_update.b, st));
    HIPCHK(h, hipMemcpyAsync(row_it, d_rows, (size_t)n_ckt * SPICEY_FIT_ROW * sizeof(double), hipMemcpyDeviceToHost, st));
    if (x) HIPCHK(h, hipMemcpy2DAsync(x_nom.data(), (size_t)n_scalar * sizeof(double), d_x, (size_t)W * n_scalar * sizeof(double), (size_t)n_scalar * sizeof(double),
                                      (size_t)n_ckt, hipMemcpyDeviceToHost, st));
    const std::vector<int32_t> was = done;
    HIPCHK(h, hipMemcpyAsync(done.data(), d_done, (size_t)n_ckt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    double ms = 0.0;
    StreamTimers::elapsed(ev_design.a, ev_design.b, &ms);
    h->last_fit_ms += ms;
    ms = 0.0;
    StreamTimers::elapsed(ev_update.a, ev_update.b, &ms);
    h->last_fit_ms += ms;
    h->last_fit_tran_ms += h->last_ms;
    bool all = true;
    for (int32_t c = 0; c < n_ckt; c++) {
      if (was[(size_t)c] == 0) {
        const double *row = row_it + (size_t)c * SPICEY_FIT_ROW;
        n_iter[c]++;
        if (row[4] != 2.0) F[c] = row[1];
        if (x && row[3] == 1.0) memcpy(x + (size_t)c * n_scalar, x_nom.data() + (size_t)c * n_scalar, (size_t)n_scalar * sizeof(double));
      }
      all = all && done[(size_t)c] != 0;
    }
    if (all) break;
  }
  for (int32_t c = 0; c < n_ckt; c++) status[c] = done[(size_t)c] == 0 ? 1 : done[(size_t)c] == 1 ? 0 : done[(size_t)c];
  // the best evaluated point: g_good of the circuits' state (a circuit whose first nominal was not evaluable keeps its start)
  SpiceyFitLayout l;
  spicey_fit_layout(n_ckt, nA, n_scalar, l);
  std::vector<double> best((size_t)n_ckt * nA);
  HIPCHK(h, restore());
  at_exit.armed = false;
  HIPCHK(h, hipMemcpy2DAsync(best.data(), (size_t)nA * sizeof(double), (const char *)(uint8_t *)d_work + l.off_state + ((size_t)nA * nA + nA) * sizeof(double),
                             (size_t)spicey_fit_state_doubles(nA) * sizeof(double), (size_t)nA * sizeof(double), (size_t)n_ckt, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  for (int32_t c = 0; c < n_ckt; c++)
    if (status[c] != 2) memcpy(g + (size_t)c * nA, best.data() + (size_t)c * nA, (size_t)nA * sizeof(double));
  if (const int32_t rc0 = r.copy_out(h, nullptr, nullptr, iters); rc0 != SPICEY_OK) return rc0;
  if (!run_err.empty()) h->err = run_err;
  return SPICEY_OK;
}

extern "C" double spicey_last_fit_ms(SpiceyHandle *h) { return h ? h->last_fit_ms : 0.0; }
extern "C" double spicey_last_fit_tran_ms(SpiceyHandle *h) { return h ? h->last_fit_tran_ms : 0.0; }
