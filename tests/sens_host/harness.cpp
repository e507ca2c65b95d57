// CPU harness of the AC sensitivity analysis (TEST INFRASTRUCTURE ONLY): the reduction of sens_exec.h — the code the kernels of
// spicey_amd/csrc/sens.hip run — through an emulation of their mapping: per (instance, frequency) 64 lanes run
// spicey_sens_lane, the partials of each of the four sums meet by s[l] += s[l + stride] for stride = 32 .. 1, lane 0 writes the
// row; then one "thread" per (instance, element) runs spicey_sens_peak.  The call is judged by spicey_sens_judge of sens.h, the
// judge of the library's entry points.  Compiled with -ffp-contract=off like the kernels' translation unit, so the results are
// the GPU's bit for bit.  d_spec and d_full start as NaNs: a row read before it was written shows.
//
// The two sweeps the reduction reads come from the injected host sweep of tests/noise_host (the host form of ac_exec.h), which
// this analysis uses as it is: pysens.py calls it for sweep D and for sweep X.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>

#include "../../spicey_amd/csrc/sens.h"

extern "C" int64_t spicey_sens_host_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE) { return spicey_sens_workspace_bytes(n_inst, n_freq, nE); }
extern "C" int32_t spicey_sens_host_req_bytes(void) { return (int32_t)sizeof(SpiceyAcSensReq); }

// have_out = 0 stands for null result buffers, work_bytes = -1 for a workspace of exactly the size needed; full may be null.
// Returns SPICEY_OK or SPICEY_ERR_BAD_DESC (text in err; the results untouched).
extern "C" int32_t spicey_sens_host_run(int32_t n_inst, int64_t n_freq, const double *v, int32_t n_v, const double *id, const double *ix, int32_t n_i, const double *R,
                                        const double *Cv, const double *Lv, const double *tol, const double *freqs, const SpiceyAcSensReq *req, double *spec,
                                        double *peak, double *full, int32_t have_out, int64_t work_bytes, char *err, int32_t err_cap) {
  std::string e;
  SpiceySensArgs A;
  const int64_t need = req ? spicey_sens_workspace_bytes(n_inst, n_freq, req->nR + req->nC + req->nL) : 0;
  if (!spicey_sens_judge(n_inst, n_freq, v, n_v, id, ix, n_i, R, Cv, Lv, tol, freqs, req, have_out != 0 && spec && peak, work_bytes < 0 ? need : work_bytes, A, e)) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  A.tol = tol;
  const int64_t slots = (int64_t)n_inst * n_freq, nE = (int64_t)A.nR + A.nC + A.nL;
  for (int64_t s = 0; s < slots * SPICEY_SENS_SPEC; s++) spec[s] = std::numeric_limits<double>::quiet_NaN();
  if (full)
    for (int64_t s = 0; s < slots * nE * 2; s++) full[s] = std::numeric_limits<double>::quiet_NaN();
  for (int64_t slot = 0; slot < slots; slot++) {
    double s[SPICEY_SENS_LANES][4];
    for (int l = 0; l < SPICEY_SENS_LANES; l++) spicey_sens_lane(A, slot, l, full, s[l]);
    for (int stride = SPICEY_SENS_LANES / 2; stride > 0; stride >>= 1)
      for (int l = 0; l < stride; l++)
        for (int j = 0; j < 4; j++) s[l][j] = s[l][j] + s[l + stride][j];
    spicey_sens_spec_row(A, slot, s[0], spec);
  }
  for (int64_t idx = 0; idx < (int64_t)n_inst * nE; idx++) spicey_sens_peak(A, idx, peak);
  return SPICEY_OK;
}
