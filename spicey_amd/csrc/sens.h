// sens.h — the host side of the sensitivity pass: validation and the workspace layout (sens_exec.h holds the arithmetic and the
// mapping).  Plain C++, shared by spicey_abi.cpp, ac_abi.cpp, sens.hip and the CPU harness of tests/sens_host; the launcher of
// sens.hip is declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

#include "../../include/spicey_hip.h"
#include "sens_exec.h"

// the request record at the head of the workspace, the tolerances [nE] behind it; -1 for arguments no launch accepts
inline int64_t spicey_sens_tol_offset() { return spicey_meas_align((int64_t)sizeof(SpiceySensArgs)); }
inline int64_t spicey_sens_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE) {
  if (n_inst <= 0 || n_freq <= 0 || nE <= 0) return -1;
  return spicey_sens_tol_offset() + spicey_meas_align((int64_t)nE * (int64_t)sizeof(double));
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing).  tol is a HOST array.  true: `A`
// is the kernels' record, buffers included, except A.tol, which the launcher points into the workspace.
inline bool spicey_sens_judge(int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_id, const double *d_ix, int32_t n_i, const double *d_R,
                              const double *d_C, const double *d_L, const double *tol, const double *d_freqs, const SpiceyAcSensReq *req, bool have_out,
                              int64_t work_bytes, SpiceySensArgs &A, std::string &err) {
  const char *what = nullptr;
  int64_t k1 = 0;
  if (!req) what = "null request";
  else if (req->struct_bytes != (int64_t)sizeof(SpiceyAcSensReq)) what = "struct_bytes is not sizeof(SpiceyAcSensReq)";
  else if (n_inst <= 0 || n_freq <= 0 || n_v <= 0 || n_i <= 0) what = "bad counts (n_inst, n_freq, n_v, n_i >= 1)";
  else if (req->nR < 0 || req->nC < 0 || req->nL < 0) what = "bad counts (nR, nC, nL >= 0)";
  else if (req->nR == 0 && req->nC == 0 && req->nL == 0) what = "no element (nR + nC + nL = 0)";
  else if ((int64_t)req->nR + req->nC + req->nL > n_i) what = "nR + nC + nL exceeds the columns of the current buffers";
  else if (!d_v || !d_id || !d_ix || !tol || !d_freqs || !have_out || (req->nR && !d_R) || (req->nC && !d_C) || (req->nL && !d_L)) what = "null buffer";
  else if (req->reserved != 0) what = "reserved must be 0";
  else if (req->out_p < -1 || req->out_p >= n_v || req->out_n < -1 || req->out_n >= n_v) what = "column out of range";
  else if (req->out_p == req->out_n) what = "the output pair names one node twice (or ground twice)";
  else {
    const int32_t nE = req->nR + req->nC + req->nL;
    k1 = req->k_to == -1 ? n_freq - 1 : req->k_to;
    if (req->k_from < 0 || k1 < 0 || k1 >= n_freq || req->k_from > k1) what = "window outside [0, n_freq) or k_from > k_to";
    else if (work_bytes < spicey_sens_workspace_bytes(n_inst, n_freq, nE)) what = "workspace too small (spicey_ac_sens_workspace_bytes)";
    else
      for (int32_t e = 0; e < nE && !what; e++)
        if (!(tol[e] >= 0.0) || !std::isfinite(tol[e])) what = "a tolerance must be finite and >= 0";
  }
  if (what) {
    err = std::string("sens: ") + what;
    return false;
  }
  A = SpiceySensArgs{d_v, d_id, d_ix, d_R, d_C, d_L, nullptr, d_freqs, n_freq, req->k_from, k1, n_inst, req->nR, req->nC, req->nL, n_i, n_v, req->out_p, req->out_n};
  return true;
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The two kernels of the sensitivity pass, enqueued on `st` behind a copy of `A` (HOST, from spicey_sens_judge) and of tol
// (HOST [nE]) into the head of d_work.  d_full may be null.  The device must be current.  No synchronisation.
hipError_t spicey_launch_sens(int device, const SpiceySensArgs &A, const double *tol, double *d_spec, double *d_peak, double *d_full, void *d_work, hipStream_t st);
#endif
