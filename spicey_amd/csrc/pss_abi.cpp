// pss_abi.cpp — spicey_run_pss of include/spicey_hip.h: the shooting-Newton loop on a handle.  Per iteration the design writes
// the handle's own state arrays, ONE transient of m_steps - 1 steps runs from them into scratch outputs of this call, and the
// update reads the end states where the run left them; only the [n_ckt][8] rows and the done flags come back per iteration.
// Every engine starts from and ends in h->state (spicey_abi.cpp, run_device_src), so every handle of spicey_create is served;
// the transient is synchronised before the update is enqueued, so a group-mode launch that spicey_sync repeats is repeated
// before its end states are read, and the update knows the instances' statuses.
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "tran_handle.h"
#include "pss.h"

namespace {
// [n_ckt][n] of the nominal instances' rows out of [n_ckt W][n], device to device on st.
hipError_t gather_nominal(void *dst, const void *src, size_t elem, int32_t n, int32_t W, int32_t n_ckt, hipStream_t st) {
  if (!n) return hipSuccess;
  return hipMemcpy2DAsync(dst, (size_t)n * elem, src, (size_t)W * n * elem, (size_t)n * elem, (size_t)n_ckt, hipMemcpyDeviceToDevice, st);
}
}  // namespace

extern "C" int32_t spicey_run_pss(SpiceyHandle *h, int64_t m_steps, double dt, const double *src_table, int32_t src_per_inst, const SpiceyPssReq *req, double *x,
                                  int32_t *on, double *history, int32_t *n_iter, int32_t *status) {
  if (!h) return SPICEY_ERR_BAD_DESC;
  const SpiceyProg &P = h->hp.hdr;
  h->last_pss_ms = h->last_pss_tran_ms = 0.0;
  forget_last_run(h);
  char buf[192];
  const char *what = spicey_pss_judge_req(req, P.nC, P.nL, P.nD, P.nS, true, buf, sizeof(buf));
  const int32_t nX = P.nC + P.nL + P.nD, ni = h->plan.n_inst;
  if (what) {
  } else if (!x || !history || !n_iter || !status || (P.nS && !on) || (P.nV && !src_table)) what = "null buffer";
  else if ((int64_t)ni != (int64_t)req->n_ckt * spicey_pss_width(req->method, nX)) {
    snprintf(buf, sizeof(buf), "the handle has %d instances, n_ckt W = %lld are needed (W = %d)", ni, (long long)req->n_ckt * spicey_pss_width(req->method, nX),
             spicey_pss_width(req->method, nX));
    what = buf;
  } else if (m_steps < 1) what = "m_steps must be >= 1";
  else if (src_per_inst != 0 && src_per_inst != 1) what = "src_per_inst must be 0 (one shared table) or 1 (one table per instance)";
  if (what) { h->err = std::string("pss: ") + what; return SPICEY_ERR_BAD_DESC; }
  const int32_t n_ckt = req->n_ckt, W = spicey_pss_width(req->method, nX);
  for (int32_t c = 0; c < n_ckt; c++) { n_iter[c] = 0; status[c] = 1; }
  HIPCHK(h, hipSetDevice(h->device));
  if (h->pending) {  // (a run still in flight: its end state is where this one starts)
    const int32_t rc0 = spicey_sync(h);
    forget_last_run(h);
    if (rc0 != SPICEY_OK && rc0 != SPICEY_ERR_SINGULAR) return rc0;
  }
  Roctx range_run("spicey_run_pss");
  hipStream_t st = h->q.stream;
  const StatePtrs S = h->state.ptrs();
  DevBuf<double> d_base, d_h, d_rows;
  DevBuf<int32_t> d_base_on, d_done;
  DevBuf<uint8_t> d_work;
  const int64_t work_bytes = spicey_pss_bytes(n_ckt, nX, req->method);
  HIPCHK(h, d_base.alloc((size_t)n_ckt * nX));
  HIPCHK(h, d_h.alloc((size_t)n_ckt * nX));
  HIPCHK(h, d_rows.alloc((size_t)n_ckt * SPICEY_PSS_ROW));
  HIPCHK(h, d_base_on.alloc(std::max<size_t>(1, (size_t)n_ckt * P.nS)));
  HIPCHK(h, d_done.alloc((size_t)n_ckt));
  HIPCHK(h, d_work.alloc((size_t)work_bytes));
  HIPCHK(h, hipMemsetAsync(d_rows, 0, (size_t)n_ckt * SPICEY_PSS_ROW * sizeof(double), st));
  HIPCHK(h, hipMemsetAsync(d_done, 0, (size_t)n_ckt * sizeof(int32_t), st));
  // the base starts as instance c W's current state: [C | L | D] side by side
  double *const base = d_base;
  const struct { double *dst; const double *src; int32_t n; } kinds[] = {{base, S.Cv, P.nC}, {base + P.nC, S.Li, P.nL}, {base + P.nC + P.nL, S.Dv, P.nD}};
  for (const auto &k : kinds)
    if (k.n)
      HIPCHK(h, hipMemcpy2DAsync(k.dst, (size_t)nX * sizeof(double), k.src, (size_t)W * k.n * sizeof(double), (size_t)k.n * sizeof(double), (size_t)n_ckt,
                                 hipMemcpyDeviceToDevice, st));
  HIPCHK(h, gather_nominal(d_base_on, S.Son, sizeof(int32_t), P.nS, W, n_ckt, st));
  SpiceyPssArgs A;
  if (!spicey_pss_judge(true, P.nC, P.nL, P.nD, P.nS, req, 1, d_base, d_base_on, d_h, S.Cv, S.Li, S.Dv, S.Son, nullptr, d_rows, d_done, true, work_bytes, A, h->err))
    return SPICEY_ERR_BAD_DESC;
  SpiceyPssArgs A_plain = A;  // the last design: every instance gets the base alone
  A_plain.perturb = 0;
  std::vector<int32_t> done((size_t)n_ckt, 0), ist((size_t)ni, 0);
  int32_t rc = check_structure(h);
  if (rc == SPICEY_ERR_SINGULAR) {  // (every nominal run would fail in its first solve)
    for (int32_t c = 0; c < n_ckt; c++) status[c] = 2;
  } else {
    HostRun r;
    if (const int32_t rc0 = r.stage(h, m_steps - 1, src_table, src_per_inst, false, false); rc0 != SPICEY_OK) return rc0;
    EventPair ev_design, ev_update;
    HIPCHK(h, ev_design.create());
    HIPCHK(h, ev_update.create());
    for (int32_t it = 0; it < req->max_iter; it++) {
      HIPCHK(h, hipEventRecord(ev_design.a, st));
      HIPCHK(h, spicey_launch_pss_design(h->device, A, d_work, st));
      HIPCHK(h, hipEventRecord(ev_design.b, st));
      rc = run_device_src(h, m_steps - 1, dt, r.d_src, src_per_inst, r.d_v, nullptr, nullptr, st, nullptr);
      if (rc != SPICEY_OK) return rc;
      rc = spicey_sync(h);
      if (rc != SPICEY_OK && rc != SPICEY_ERR_SINGULAR) return rc;
      const std::string run_err = h->err;
      const bool any_bad = spicey_last_inst_status(h, ist.data()) > 0;
      HIPCHK(h, hipEventRecord(ev_update.a, st));
      HIPCHK(h, spicey_launch_pss_update(h->device, A, any_bad ? ist.data() : nullptr, d_work, st));
      HIPCHK(h, hipEventRecord(ev_update.b, st));
      HIPCHK(h, hipMemcpyAsync(history + (size_t)it * n_ckt * SPICEY_PSS_ROW, d_rows, (size_t)n_ckt * SPICEY_PSS_ROW * sizeof(double), hipMemcpyDeviceToHost, st));
      for (int32_t c = 0; c < n_ckt; c++) n_iter[c] += done[(size_t)c] == 0;
      HIPCHK(h, hipMemcpyAsync(done.data(), d_done, (size_t)n_ckt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      double ms = 0.0;
      StreamTimers::elapsed(ev_design.a, ev_design.b, &ms);
      h->last_pss_ms += ms;
      ms = 0.0;
      StreamTimers::elapsed(ev_update.a, ev_update.b, &ms);
      h->last_pss_ms += ms;
      h->last_pss_tran_ms += h->last_ms;
      if (rc == SPICEY_ERR_SINGULAR) h->err = run_err;
      bool all = true;
      for (int32_t c = 0; c < n_ckt; c++) all = all && done[(size_t)c] != 0;
      if (all) break;
    }
    for (int32_t c = 0; c < n_ckt; c++) status[c] = done[(size_t)c] == 0 ? 1 : done[(size_t)c] == 1 ? 0 : done[(size_t)c];
  }
  // every instance of circuit c holds base[c] and base_on[c]: spicey_get_state is defined
  HIPCHK(h, spicey_launch_pss_design(h->device, A_plain, d_work, st));
  HIPCHK(h, hipMemcpyAsync(x, d_base, (size_t)n_ckt * nX * sizeof(double), hipMemcpyDeviceToHost, st));
  if (P.nS) HIPCHK(h, hipMemcpyAsync(on, d_base_on, (size_t)n_ckt * P.nS * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return SPICEY_OK;
}

extern "C" double spicey_last_pss_ms(SpiceyHandle *h) { return h ? h->last_pss_ms : 0.0; }
extern "C" double spicey_last_pss_tran_ms(SpiceyHandle *h) { return h ? h->last_pss_tran_ms : 0.0; }
