// CPU harness of the element sizing (TEST INFRASTRUCTURE ONLY): the design and the update of fit_exec.h — the code the kernels of
// spicey_amd/csrc/fit.hip run — through an emulation of their mapping: one "thread" per (instance, element) runs
// spicey_fit_design; per circuit an emulated workgroup of `threads` threads runs spicey_fit_update, every phase in all its
// threads in turn (the highest first: nothing may depend on the order) with the barrier behind it, the pivot search in 64 lanes
// met at stride 32 .. 1 as the device's first wave meets them.  The calls are judged by the judges of fit.h, those of the
// library's entry points, and run on the CALLER's workspace, laid out as the launchers lay out the device's: it carries the
// circuits' state from one update to the next.  Compiled with -ffp-contract=off like the kernels' translation unit, so the
// results are the GPU's bit for bit.
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/fit.h"

namespace {
int32_t refuse(const std::string &e, char *err, int32_t err_cap) {
  if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
  return SPICEY_ERR_BAD_DESC;
}

struct HostWorkgroup {
  int32_t T;
  template <class F>
  void par(F f) {
    for (int32_t t = T - 1; t >= 0; t--) f(t);
  }
  void pivot(const SpiceyFitArgs &A, const double *M, int32_t k, SpiceyFitShared *sh) {
    SpiceyPssPiv p[SPICEY_FIT_LANES];
    for (int32_t l = SPICEY_FIT_LANES - 1; l >= 0; l--) p[l] = spicey_pss_piv_lane(M, A.nA, k, l);
    for (int stride = SPICEY_FIT_LANES / 2; stride > 0; stride >>= 1)
      for (int l = 0; l < stride; l++) spicey_pss_piv_meet(&p[l], p[l + stride]);
    spicey_fit_piv_done(A, sh, k, p[0]);
  }
};
}  // namespace

extern "C" int64_t spicey_fit_host_workspace_bytes(int32_t n_ckt, int32_t nA, int32_t n_scalar) { return spicey_fit_bytes(n_ckt, nA, n_scalar); }
extern "C" int32_t spicey_fit_host_req_bytes(void) { return (int32_t)sizeof(SpiceyFitReq); }
extern "C" int32_t spicey_fit_host_goal_bytes(void) { return (int32_t)sizeof(SpiceyFitGoal); }
extern "C" int64_t spicey_fit_host_lds_bytes(int32_t nA) { return (int64_t)spicey_fit_lds_bytes(nA); }
// Where the circuits' state begins in the workspace, and its doubles per circuit.
extern "C" int64_t spicey_fit_host_state_offset(int32_t n_ckt, int32_t nA, int32_t n_scalar) {
  SpiceyFitLayout l;
  return spicey_fit_layout(n_ckt, nA, n_scalar, l) ? l.off_state : -1;
}
extern "C" int64_t spicey_fit_host_state_doubles(int32_t nA) { return spicey_fit_state_doubles(nA); }

// work: the caller's workspace of work_bytes bytes (null stands for a null workspace).  Returns SPICEY_OK or SPICEY_ERR_BAD_DESC
// (text in err; the results untouched).
extern "C" int32_t spicey_fit_host_design(int32_t nR, int32_t nC, int32_t nL, const double *R, const double *C, const double *L, const SpiceyFitReq *req,
                                          const int32_t *act, const double *step, const double *g, double *oR, double *oC, double *oL, char *work, int64_t work_bytes,
                                          char *err, int32_t err_cap) {
  std::string e;
  SpiceyFitArgs A;
  if (!spicey_fit_design_judge(nR, nC, nL, R, C, L, req, act, step, g, oR, oC, oL, work != nullptr, work_bytes, A, e)) return refuse(e, err, err_cap);
  SpiceyFitLayout l{};
  spicey_fit_layout(A.n_ckt, A.nA, 1, l);
  spicey_fit_design_head(l, A, act, step, work, work);
  const int64_t total = l.n_inst * ((int64_t)nR + nC + nL);
  for (int64_t idx = 0; idx < total; idx++) spicey_fit_design(*(const SpiceyFitArgs *)work, idx);
  return SPICEY_OK;
}

// threads: the emulated workgroup (0: 256).
extern "C" int32_t spicey_fit_host_update(const SpiceyFitReq *req, int32_t n_scalar, int32_t first, const double *step, const double *g_lo, const double *g_hi,
                                          const SpiceyFitGoal *goals, const uint8_t *valid, const double *x, double *g, double *rows, int32_t *done, char *work,
                                          int64_t work_bytes, int32_t threads, char *err, int32_t err_cap) {
  std::string e;
  SpiceyFitArgs A;
  if (!spicey_fit_update_judge(req, n_scalar, first, step, g_lo, g_hi, goals, x, g, rows, done, work != nullptr, work_bytes, A, e)) return refuse(e, err, err_cap);
  SpiceyFitLayout l{};
  spicey_fit_layout(A.n_ckt, A.nA, A.n_scalar, l);
  spicey_fit_update_head(l, A, step, g_lo, g_hi, goals, valid, work + l.off_rec, work);
  // (the matrix: exactly the bytes of the device's dynamic LDS, so a sanitizer sees an access past them)
  std::vector<double> M(spicey_fit_lds_bytes(A.nA) / sizeof(double));
  HostWorkgroup wg{threads > 0 ? threads : SPICEY_FIT_THREADS};
  for (int32_t c = 0; c < A.n_ckt; c++) {
    SpiceyFitShared sh;
    memset(&sh, 0x5a, sizeof(sh));  // (LDS is not cleared between workgroups)
    spicey_fit_update(A, c, M.data(), &sh, wg);
  }
  return SPICEY_OK;
}
