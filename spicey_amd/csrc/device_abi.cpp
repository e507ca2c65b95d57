// device_abi.cpp — the handle-less entry points of include/spicey_hip.h: per reduction a spicey_*_workspace_bytes and a
// spicey_*_device that judges the call (a refusal launches nothing and leaves its text in the calling thread's error), opens
// the device and enqueues the launch on the caller's stream and buffers.
#include <hip/hip_runtime_api.h>

#include <functional>
#include <string>
#include <vector>

#include "tran_handle.h"
#include "ac_measure.h"
#include "ac_measure_exec.h"
#include "fit.h"
#include "fourier.h"
#include "fourier_exec.h"
#include "measure.h"
#include "measure_exec.h"
#include "noise.h"
#include "mc.h"
#include "sens.h"
#include "power.h"
#include "pss.h"
#include "values.h"
#include "spectrum.h"
#include "timing.h"
#include "timing_exec.h"
#include "tran_mc.h"
#include "tran_sens.h"

// Waveform measurements (include/spicey_hip.h): the reduction pass of measure.hip on any device buffers, no handle.
extern "C" int64_t spicey_measure_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  return spicey_meas_workspace_bytes(n_inst, n_points, n_req);
}

// The tail of the handle-less spicey_*_device entry points, behind their judge: the device opened, the launch enqueued, a
// failure as "<launcher>: <the runtime's text>" in the calling thread's error.
static int32_t launch_on_device(int32_t device, const char *launcher, const std::function<hipError_t()> &launch) {
  int ncu = 0;
  if (const int32_t rc = spicey_open_device(device, &ncu, g_err); rc != SPICEY_OK) return rc;
  const hipError_t e = launch();
  if (e != hipSuccess) { g_err = std::string(launcher) + ": " + hipGetErrorString(e); return SPICEY_ERR_HIP; }
  return SPICEY_OK;
}

extern "C" int32_t spicey_measure_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                         int32_t n_i, const SpiceyMeasReq *reqs, int32_t n_req, double *d_meas, void *d_work, int64_t work_bytes,
                                         void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  std::vector<SpiceyMeasDevReq> table;
  if (const int32_t rc = spicey_judge_measure("measure", spicey_meas_plan, spicey_meas_workspace_bytes, n_inst, n_points, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs,
                                              n_req, d_meas && d_work, work_bytes, table, g_err); rc != SPICEY_OK)
    return rc;
  return launch_on_device(device, "spicey_launch_measure", [&]() {
    return spicey_launch_measure(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, table.data(), n_req, d_meas, d_work, (hipStream_t)stream);
  });
}

// Edge timing (include/spicey_hip.h): the reduction of timing.hip on any device buffers, no handle.
extern "C" int64_t spicey_timing_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyTimingReq *reqs, int32_t n_req) {
  return spicey_tim_workspace_bytes(n_inst, n_points, reqs, n_req);
}

extern "C" int32_t spicey_timing_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                        int32_t n_i, const SpiceyTimingReq *reqs, int32_t n_req, double *d_out, void *d_work, int64_t work_bytes,
                                        void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyTimPlan plan;
  if (!spicey_tim_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_timing", [&]() {
    return spicey_launch_timing(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan, d_out, d_work, (hipStream_t)stream);
  });
}

// Spectrum (include/spicey_hip.h): the FFT pass of spectrum.hip on any device buffers, no handle.
extern "C" int64_t spicey_spectrum_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceySpecReq *reqs, int32_t n_req) {
  return spicey_spec_workspace_bytes(n_inst, n_points, reqs, n_req);
}

extern "C" int32_t spicey_spectrum_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                          int32_t n_i, const SpiceySpecReq *reqs, int32_t n_req, double *d_out, int32_t out_stride, void *d_work,
                                          int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceySpecPlan plan;
  if (!spicey_spec_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, out_stride, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_spectrum", [&]() {
    return spicey_launch_spectrum(device, n_inst, n_points, d_v, n_v, d_i, n_i, plan, d_out, out_stride, d_work, (hipStream_t)stream);
  });
}

// Products of two signals (include/spicey_hip.h): the reduction of power.hip on any device buffers, no handle.
extern "C" int64_t spicey_power_workspace_bytes(int32_t n_inst, int64_t n_points, int32_t n_req) {
  return spicey_pow_workspace_bytes(n_inst, n_points, n_req);
}

extern "C" int32_t spicey_power_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                       int32_t n_i, const SpiceyPowerReq *reqs, int32_t n_req, double *d_out, void *d_work, int64_t work_bytes,
                                       void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  std::vector<SpiceyPowerDevReq> table;
  if (!spicey_power_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, work_bytes, table, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_power", [&]() {
    return spicey_launch_power(device, n_inst, n_points, d_v, n_v, d_i, n_i, table.data(), n_req, d_out, d_work, (hipStream_t)stream);
  });
}

// Waveform values (include/spicey_hip.h): the pass of values.hip on any device buffers, no handle.
extern "C" int64_t spicey_values_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyValReq *reqs, int32_t n_req, int64_t n_pts) {
  return spicey_val_workspace_bytes(n_inst, n_points, reqs, n_req, n_pts);
}

extern "C" int32_t spicey_values_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                        int32_t n_i, const SpiceyValReq *reqs, int32_t n_req, const SpiceyValPoint *pts, int64_t n_pts, const double *d_timing,
                                        int32_t n_timing, double *d_out, int32_t out_stride, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyValPlan plan;
  if (!spicey_val_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, pts, n_pts, d_timing != nullptr, n_timing, d_out && d_work,
                        out_stride, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_values", [&]() {
    return spicey_launch_values(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan, pts, d_timing, n_timing, d_out, out_stride, d_work, (hipStream_t)stream);
  });
}

// Harmonics (include/spicey_hip.h): the reduction of fourier.hip on any device buffers, no handle.
extern "C" int64_t spicey_fourier_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyFourReq *reqs, int32_t n_req) {
  return spicey_four_workspace_bytes(n_inst, n_points, reqs, n_req);
}

extern "C" int32_t spicey_fourier_device(int32_t device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i,
                                         int32_t n_i, const SpiceyFourReq *reqs, int32_t n_req, double *d_out, int32_t out_stride, void *d_work,
                                         int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyFourPlan plan;
  if (!spicey_four_judge(n_inst, n_points, dt, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs, n_req, d_out && d_work, out_stride, work_bytes, plan, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_fourier", [&]() {
    return spicey_launch_fourier(device, n_inst, n_points, dt, d_v, n_v, d_i, n_i, plan, d_out, out_stride, d_work, (hipStream_t)stream);
  });
}

// The same for an AC sweep's complex buffers (include/spicey_hip.h): the reduction of ac_measure.hip, no handle.
extern "C" int64_t spicey_ac_measure_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t n_req) {
  return spicey_acm_workspace_bytes(n_inst, n_freq, n_req);
}

extern "C" int32_t spicey_ac_measure_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                            const SpiceyAcMeasReq *reqs, int32_t n_req, double *d_meas, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  std::vector<SpiceyAcMeasDevReq> table;
  if (const int32_t rc = spicey_judge_measure("ac measure", spicey_acm_plan, spicey_acm_workspace_bytes, n_inst, n_freq, d_v != nullptr, n_v, d_i != nullptr, n_i, reqs,
                                              n_req, d_meas && d_work, work_bytes, table, g_err); rc != SPICEY_OK)
    return rc;
  return launch_on_device(device, "spicey_launch_ac_measure", [&]() {
    return spicey_launch_ac_measure(device, n_inst, n_freq, d_v, n_v, d_i, n_i, table.data(), n_req, d_meas, d_work, (hipStream_t)stream);
  });
}

// Thermal noise of an injected AC sweep (include/spicey_hip.h): the reduction of noise.hip on any device buffers, no handle.
extern "C" int64_t spicey_ac_noise_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nR) { return spicey_noise_workspace_bytes(n_inst, n_freq, nR); }

extern "C" int32_t spicey_ac_noise_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                          const double *d_R, int32_t nR, const double *d_freqs, const SpiceyAcNoiseReq *req, double *d_spec, double *d_contrib,
                                          double *d_total, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyNoiseArgs A;
  if (!spicey_noise_judge(n_inst, n_freq, d_v, n_v, d_i, n_i, d_R, nR, d_freqs, req, d_spec && d_contrib && d_total && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_noise", [&]() { return spicey_launch_noise(device, A, d_spec, d_contrib, d_total, d_work, (hipStream_t)stream); });
}

// AC sensitivities of a direct and an adjoint sweep (include/spicey_hip.h): the reduction of sens.hip on any device buffers, no
// handle.  tol is a HOST array: judged here, uploaded through the workspace.
extern "C" int64_t spicey_ac_sens_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE) { return spicey_sens_workspace_bytes(n_inst, n_freq, nE); }

extern "C" int32_t spicey_ac_sens_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v_dir, int32_t n_v, const double *d_i_dir,
                                         const double *d_i_adj, int32_t n_i, const double *d_R, const double *d_C, const double *d_L, const double *tol,
                                         const double *d_freqs, const SpiceyAcSensReq *req, double *d_spec, double *d_peak, double *d_full, void *d_work,
                                         int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceySensArgs A;
  if (!spicey_sens_judge(n_inst, n_freq, d_v_dir, n_v, d_i_dir, d_i_adj, n_i, d_R, d_C, d_L, tol, d_freqs, req, d_spec && d_peak && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_sens", [&]() { return spicey_launch_sens(device, A, tol, d_spec, d_peak, d_full, d_work, (hipStream_t)stream); });
}

extern "C" int64_t spicey_ac_mc_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE, int32_t log2K, int32_t n_rank) {
  return spicey_mc_workspace_bytes(n_inst, n_freq, nE, log2K, n_rank);
}

extern "C" int32_t spicey_ac_mc_draw_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                            const double *d_L, const double *tol, const double *icdf, const SpiceyAcMcReq *req, double *d_Rinv_out,
                                            double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyMcDrawArgs A;
  if (!spicey_mc_draw_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, tol, icdf, req, d_Rinv_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_mc_draw", [&]() { return spicey_launch_mc_draw(device, A, tol, icdf, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_ac_mc_reduce_device(int32_t device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const uint8_t *valid,
                                              const double *lo, const double *hi, const int64_t *ranks, int32_t n_rank, const SpiceyAcMcReq *req,
                                              int64_t *d_sample, double *d_freq, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyMcReduceArgs A;
  if (!spicey_mc_reduce_judge(n_inst, n_freq, d_v, n_v, valid, ranks, n_rank, req, d_sample && d_freq && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_mc_reduce",
                          [&]() { return spicey_launch_mc_reduce(device, A, valid, lo, hi, ranks, d_sample, d_freq, d_work, (hipStream_t)stream); });
}

// Monte Carlo of transient runs (include/spicey_hip.h): the draw and the reduction of tran_mc.hip on any device buffers, no handle.
extern "C" int64_t spicey_tran_mc_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t log2K, int32_t n_prob) {
  return spicey_tmc_workspace_bytes(n_inst, n_scalar, nE, log2K, n_prob);
}

extern "C" int32_t spicey_tran_mc_draw_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                              const double *d_L, const double *tol, const double *icdf, const SpiceyTranMcReq *req, double *d_R_out,
                                              double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyMcDrawArgs A;
  if (!spicey_tmc_draw_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, tol, icdf, req, d_R_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_tmc_draw", [&]() { return spicey_launch_tmc_draw(device, A, tol, icdf, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_tran_mc_reduce_device(int32_t device, int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                                const uint8_t *valid, const double *lo, const double *hi, const double *probs, int32_t n_prob, double *d_x,
                                                double *d_stat, int64_t *d_sample, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyTmcArgs A;
  if (!spicey_tmc_reduce_judge(n_inst, rows, scalars, n_scalar, lo, hi, probs, n_prob, d_x && d_stat && d_sample && d_work, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_tmc_reduce", [&]() {
    return spicey_launch_tmc_reduce(device, A, scalars, valid, lo, hi, probs, d_x, d_stat, d_sample, d_work, (hipStream_t)stream);
  });
}

// Sensitivities and corners of transient measurements (include/spicey_hip.h): the design and the reduction of tran_sens.hip on any
// device buffers, no handle.
extern "C" int64_t spicey_tran_sens_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t nA) {
  return spicey_ts_workspace_bytes(n_inst, n_scalar, nE, nA);
}

extern "C" int32_t spicey_tran_sens_design_device(int32_t device, int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C,
                                                  const double *d_L, const SpiceyTranSensReq *req, const int32_t *act, const double *step, const int8_t *lvl,
                                                  const double *tol, double *d_R_out, double *d_C_out, double *d_L_out, void *d_work, int64_t work_bytes,
                                                  void *stream) {
  SpiceyTsDesignArgs A;
  if (!spicey_ts_design_judge(n_inst, nR, nC, nL, d_R, d_C, d_L, req, -1, act, step, lvl, tol, d_R_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_ts_design", [&]() { return spicey_launch_ts_design(device, A, act, step, lvl, tol, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_tran_sens_reduce_device(int32_t device, int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar,
                                                  const uint8_t *valid, const double *step, const double *tol_act, int32_t nA, double *d_x, double *d_sens,
                                                  int8_t *d_sign, double *d_bound, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyTmcArgs T;
  SpiceyTsReduceArgs A;
  if (!spicey_ts_reduce_judge(n_inst, rows, scalars, n_scalar, step, tol_act, nA, d_x && d_sens && d_sign && d_bound && d_work, work_bytes, T, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_ts_reduce", [&]() {
    return spicey_launch_ts_reduce(device, T, A, scalars, valid, step, tol_act, d_x, d_sens, d_sign, d_bound, d_work, (hipStream_t)stream);
  });
}

// Periodic steady state (include/spicey_hip.h): the design over the state and the Newton update of pss.hip on any device buffers,
// no handle.
extern "C" int64_t spicey_pss_workspace_bytes(int32_t n_ckt, int32_t nX, int32_t method) { return spicey_pss_bytes(n_ckt, nX, method); }

extern "C" int32_t spicey_pss_design_device(int32_t device, int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, int32_t perturb,
                                            const double *d_base, const int32_t *d_base_on, double *d_h, double *d_Cv, double *d_Li, double *d_Dv, int32_t *d_Son,
                                            void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyPssArgs A;
  if (!spicey_pss_judge(false, nC, nL, nD, nS, req, perturb, (double *)d_base, (int32_t *)d_base_on, d_h, d_Cv, d_Li, d_Dv, d_Son, nullptr, nullptr, nullptr,
                        d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_pss_design", [&]() { return spicey_launch_pss_design(device, A, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_pss_update_device(int32_t device, int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, const int32_t *inst_status,
                                            double *d_base, int32_t *d_base_on, const double *d_h, const double *d_Cv, const double *d_Li, const double *d_Dv,
                                            const int32_t *d_Son, double *d_delta, double *d_rows, int32_t *d_done, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyPssArgs A;
  if (!spicey_pss_judge(true, nC, nL, nD, nS, req, 1, d_base, d_base_on, (double *)d_h, (double *)d_Cv, (double *)d_Li, (double *)d_Dv, (int32_t *)d_Son, d_delta,
                        d_rows, d_done, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_pss_update", [&]() { return spicey_launch_pss_update(device, A, inst_status, d_work, (hipStream_t)stream); });
}

// Sizing elements to measured goals (include/spicey_hip.h): the design over the gains and the damped least-squares update of
// fit.hip on any device buffers, no handle.
extern "C" int64_t spicey_fit_workspace_bytes(int32_t n_ckt, int32_t nA, int32_t n_scalar) { return spicey_fit_bytes(n_ckt, nA, n_scalar); }

extern "C" int32_t spicey_fit_design_device(int32_t device, int32_t nR, int32_t nC, int32_t nL, const double *d_R, const double *d_C, const double *d_L,
                                            const SpiceyFitReq *req, const int32_t *act, const double *step, const double *d_g, double *d_R_out, double *d_C_out,
                                            double *d_L_out, void *d_work, int64_t work_bytes, void *stream) {
  // (the call is judged before the device is touched: a refusal launches nothing)
  SpiceyFitArgs A;
  if (!spicey_fit_design_judge(nR, nC, nL, d_R, d_C, d_L, req, act, step, d_g, d_R_out, d_C_out, d_L_out, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_fit_design", [&]() { return spicey_launch_fit_design(device, A, act, step, d_work, (hipStream_t)stream); });
}

extern "C" int32_t spicey_fit_update_device(int32_t device, const SpiceyFitReq *req, int32_t n_scalar, int32_t first, const double *step, const double *g_lo,
                                            const double *g_hi, const SpiceyFitGoal *goals, const uint8_t *valid, const double *d_x, double *d_g, double *d_rows,
                                            int32_t *d_done, void *d_work, int64_t work_bytes, void *stream) {
  SpiceyFitArgs A;
  if (!spicey_fit_update_judge(req, n_scalar, first, step, g_lo, g_hi, goals, d_x, d_g, d_rows, d_done, d_work != nullptr, work_bytes, A, g_err))
    return SPICEY_ERR_BAD_DESC;
  return launch_on_device(device, "spicey_launch_fit_update",
                          [&]() { return spicey_launch_fit_update(device, A, step, g_lo, g_hi, goals, valid, d_work, (hipStream_t)stream); });
}
