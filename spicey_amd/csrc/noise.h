// noise.h — the host side of the noise pass: validation and the workspace layout (noise_exec.h holds the arithmetic and the
// mapping).  Plain C++, shared by spicey_abi.cpp, ac_abi.cpp, noise.hip and the CPU harness of tests/noise_host; the
// launcher of noise.hip is declared at the end for translation units that have the HIP runtime's types.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

#include "noise_exec.h"

// the request record at the head of the workspace; -1 for arguments no launch accepts
inline int64_t spicey_noise_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nR) {
  if (n_inst <= 0 || n_freq <= 0 || nR <= 0) return -1;
  return spicey_meas_align((int64_t)sizeof(SpiceyNoiseArgs));
}

// Every refusal of a call, judged before the device is touched (a refusal launches nothing).  true: `A` is the kernels'
// record, buffers included.
inline bool spicey_noise_judge(int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i, const double *d_R, int32_t nR,
                               const double *d_freqs, const SpiceyAcNoiseReq *req, bool have_out, int64_t work_bytes, SpiceyNoiseArgs &A, std::string &err) {
  const char *what = nullptr;
  int64_t k1 = 0;
  if (!req) what = "null request";
  else if (req->struct_bytes != (int64_t)sizeof(SpiceyAcNoiseReq)) what = "struct_bytes is not sizeof(SpiceyAcNoiseReq)";
  else if (n_inst <= 0 || n_freq <= 0 || nR <= 0 || n_v <= 0 || n_i <= 0) what = "bad counts (n_inst, n_freq, nR, n_v, n_i >= 1)";
  else if (!d_v || !d_i || !d_R || !d_freqs || !have_out) what = "null buffer";
  else if (nR > n_i) what = "nR exceeds the columns of the current buffer";
  else if (req->reserved != 0) what = "reserved must be 0";
  else if (req->out_p < -1 || req->out_p >= n_v || req->out_n < -1 || req->out_n >= n_v || req->in_col < -1 || req->in_col >= n_i) what = "column out of range";
  else if (req->out_p == req->out_n) what = "the output pair names one node twice (or ground twice)";
  else if (!(req->kt4 >= 0.0) || !std::isfinite(req->kt4)) what = "kt4 must be finite and >= 0";
  else {
    k1 = req->k_to == -1 ? n_freq - 1 : req->k_to;
    if (req->k_from < 0 || k1 < 0 || k1 >= n_freq || req->k_from > k1) what = "window outside [0, n_freq) or k_from > k_to";
    else if (work_bytes < spicey_noise_workspace_bytes(n_inst, n_freq, nR)) what = "workspace too small (spicey_ac_noise_workspace_bytes)";
  }
  if (what) {
    err = std::string("noise: ") + what;
    return false;
  }
  A = SpiceyNoiseArgs{d_i, d_v, d_R, d_freqs, req->kt4, n_freq, req->k_from, k1, n_inst, nR, n_i, n_v, req->out_p, req->out_n, req->in_col, 0};
  return true;
}

#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H)
// The two kernels of the noise pass, enqueued on `st` behind a copy of `A` (HOST, from spicey_noise_judge) into the head of
// d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_noise(int device, const SpiceyNoiseArgs &A, double *d_spec, double *d_contrib, double *d_total, void *d_work, hipStream_t st);
#endif
