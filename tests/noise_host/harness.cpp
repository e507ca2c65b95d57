// CPU harness of the noise analysis (TEST INFRASTRUCTURE ONLY), two halves:
//   * the reduction: noise_exec.h — the code the kernels of spicey_amd/csrc/noise.hip run — through an emulation of their
//     mapping: per (instance, frequency) 64 lanes run spicey_noise_lane, the partials meet by s[l] += s[l + stride] for
//     stride = 32 .. 1, lane 0 writes the row; then one "thread" per (instance, row) runs spicey_noise_band.  The call is
//     judged by spicey_noise_judge of noise.h, the judge of the library's entry points.  Compiled with -ffp-contract=off like
//     the kernels' translation unit, so the results are the GPU's bit for bit.  d_spec starts as NaNs: a row read before it
//     was written shows.
//   * the injected sweep: the host form of ac_exec.h (the phase code of ac.hip) on the program of symbolic.cpp, with a small
//     executor of its own (the threads of a phase run one after the other, in either order); the injection's rows come from
//     HostProgram::rpos exactly as ac_abi.cpp forms them.  Per-solve or resident sweep, dense fallback behind both.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/symbolic.h"
#include "../../spicey_amd/csrc/ac_exec.h"
#include "../../spicey_amd/csrc/noise.h"

namespace {
struct HostExec {
  int T;
  bool reverse;
  void *rr = nullptr;  // std::vector<Regs>* of the resident sweep
  int threads() const { return T; }
  int atomic_inc(int32_t *p) { return (*p)++; }
  template <class Regs>
  Regs &regs(int tid) { return (*static_cast<std::vector<Regs> *>(rr))[(size_t)tid]; }
  template <class F>
  void phase(int, F f) {
    if (!reverse)
      for (int t = 0; t < T; t++) f(t);
    else
      for (int t = T - 1; t >= 0; t--) f(t);
  }
};

void put_err(const std::string &e, char *err, int32_t cap) {
  if (err && cap > 0) { strncpy(err, e.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
}
}  // namespace

extern "C" int64_t spicey_noise_host_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nR) { return spicey_noise_workspace_bytes(n_inst, n_freq, nR); }
extern "C" int32_t spicey_noise_host_req_bytes(void) { return (int32_t)sizeof(SpiceyAcNoiseReq); }

// have_out = 0 stands for null result buffers, work_bytes = -1 for a workspace of exactly the size needed.  Returns SPICEY_OK
// or SPICEY_ERR_BAD_DESC (text in err; the results untouched).
extern "C" int32_t spicey_noise_host_run(int32_t n_inst, int64_t n_freq, const double *v, int32_t n_v, const double *i, int32_t n_i, const double *R, int32_t nR,
                                         const double *freqs, const SpiceyAcNoiseReq *req, double *spec, double *contrib, double *total, int32_t have_out,
                                         int64_t work_bytes, char *err, int32_t err_cap) {
  std::string e;
  SpiceyNoiseArgs A;
  const int64_t need = spicey_noise_workspace_bytes(n_inst, n_freq, nR);
  if (!spicey_noise_judge(n_inst, n_freq, v, n_v, i, n_i, R, nR, freqs, req, have_out != 0 && spec && contrib && total, work_bytes < 0 ? need : work_bytes, A, e)) {
    put_err(e, err, err_cap);
    return SPICEY_ERR_BAD_DESC;
  }
  const int64_t slots = (int64_t)n_inst * n_freq;
  for (int64_t s = 0; s < slots * SPICEY_NOISE_SPEC; s++) spec[s] = std::numeric_limits<double>::quiet_NaN();
  for (int64_t slot = 0; slot < slots; slot++) {
    double s[SPICEY_NOISE_LANES];
    for (int l = 0; l < SPICEY_NOISE_LANES; l++) s[l] = spicey_noise_lane(A, slot, l);
    for (int stride = SPICEY_NOISE_LANES / 2; stride > 0; stride >>= 1)
      for (int l = 0; l < stride; l++) s[l] = s[l] + s[l + stride];
    spicey_noise_spec_row(A, slot, s[0], spec);
  }
  for (int64_t idx = 0; idx < (int64_t)n_inst * ((int64_t)nR + 2); idx++) spicey_noise_band(A, idx, spec, contrib, total);
  return SPICEY_OK;
}

// The AC sweep of `d` with the current (re, im) injected into node_p and drawn from node_n (0 = ground; both 0: none), on T
// emulated threads.  vph null: every phasor zero.  mode bit 0: the threads of a phase in reverse order; bit 1: the resident
// sweep (capacities of the device build: 12 record slots, 10 entries per thread; `stride` workgroups per instance); bit 2: no
// dense fallback.  status [n_inst * n_freq] (or null) receives the slots' words after the fallback; pos [4] (or null) the
// pivot positions {row of node_p, column of node_p, row of node_n, column of node_n}, -1 for ground; dense (or null) the
// number of solves the fallback repeated.
extern "C" int32_t spicey_noise_host_sweep(const SpiceyDesc *d, int32_t T, int64_t n_freq, const double *freqs, const double *vph, int32_t node_p, int32_t node_n,
                                           double re, double im, double *out_v, double *out_i, int32_t mode, int32_t stride, int32_t *status_out, int32_t *pos,
                                           int32_t *dense) {
  SpiceyDesc dd = *d;
  dd.nS = 0;
  dd.nD = 0;
  HostProgram hp;
  std::string err;
  const int32_t rc = spicey_build_program(&dd, hp, err, true, 0, false);
  if (rc != SPICEY_OK) return rc;
  const SpiceyProg P = hp.bind(hp.blob.data());
  if (hp.structurally_singular) return SPICEY_ERR_SINGULAR;
  if (T <= 0 || (T & 63) || node_p < 0 || node_p > d->n_nodes || node_n < 0 || node_n > d->n_nodes || (node_p == node_n && node_p != 0) || stride < 1)
    return SPICEY_ERR_BAD_DESC;
  const size_t slots = (size_t)d->n_inst * (size_t)n_freq;
  std::vector<int32_t> status(slots + 1);
  std::vector<double> rinv((size_t)d->n_inst * (size_t)d->nR), zero_ph((size_t)d->n_inst * (size_t)d->nV * 2 + 1, 0.0);
  for (size_t k = 0; k < rinv.size(); k++) rinv[k] = 1.0 / d->R_val[k];
  SpiceyAcRun R{};
  R.R_inv = rinv.data(); R.C_val = d->C_val; R.L_val = d->L_val;
  R.freqs = freqs; R.vph = vph ? vph : zero_ph.data(); R.out_v = out_v; R.out_i = out_i; R.gW = nullptr; R.status = status.data();
  R.n_freq = n_freq; R.n_inst = d->n_inst;
  if (node_p > 0) R.inj_p = 1 + P.nLU + hp.rpos[(size_t)node_p - 1];
  if (node_n > 0) R.inj_n = 1 + P.nLU + hp.rpos[(size_t)node_n - 1];
  R.inj_re = re; R.inj_im = im;
  if (pos) {
    pos[0] = node_p > 0 ? hp.rpos[(size_t)node_p - 1] : -1; pos[1] = node_p > 0 ? hp.cpos[(size_t)node_p - 1] : -1;
    pos[2] = node_n > 0 ? hp.rpos[(size_t)node_n - 1] : -1; pos[3] = node_n > 0 ? hp.cpos[(size_t)node_n - 1] : -1;
  }
  std::vector<SpiceyCx> W((size_t)P.nW + 1);
  int32_t flags[2] = {0, 0};
  const bool reverse = (mode & 1) != 0;
  if (mode & 2) {
    if (!P.has16 || P.nLU > 10 * T || T > 512) return SPICEY_ERR_BAD_DESC;
    HostResident hr;
    spicey_build_resident(hp, T, 12, hr, 0, false);
    const SpiceyResident Q = hr.bind(hr.blob.data());
    for (int in = 0; in < d->n_inst; in++)
      for (int64_t f0 = 0; f0 < stride && f0 < n_freq; f0++) {
        HostExec ex{T, reverse};
        std::vector<AcResRegs<12, 10>> regs((size_t)T);
        ex.rr = &regs;
        spicey_ac_sweep_resident<12, 10>(ex, P, Q, R, W.data(), flags, (size_t)in, f0, (int64_t)stride);
      }
  } else {
    for (size_t s = 0; s < slots; s++) {
      HostExec ex{T, reverse};
      spicey_ac_solve(ex, P, R, W.data(), flags, (int64_t)s);
    }
  }
  int32_t nd = 0;
  if (!(mode & 4)) {
    std::vector<SpiceyCx> A((size_t)P.n * ((size_t)P.n + 1));
    std::vector<double> sd((size_t)T + 2 * (size_t)P.n + 2);
    std::vector<int32_t> si((size_t)T + (size_t)P.n + 4);
    for (size_t s = 0; s < slots; s++)
      if (status[s]) {
        HostExec ex{T, reverse};
        spicey_ac_dense_solve(ex, P, R, W.data(), A.data(), sd.data(), si.data(), flags, (int64_t)s);
        nd++;
      }
  }
  if (dense) *dense = nd;
  if (status_out) memcpy(status_out, status.data(), slots * sizeof(int32_t));
  for (size_t s = 0; s < slots; s++)
    if (status[s]) return status[s] == 1 ? SPICEY_ERR_SINGULAR : SPICEY_ERR_COMPLEX_DIV;
  return SPICEY_OK;
}
