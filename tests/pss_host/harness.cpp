// CPU harness of the periodic steady state (TEST INFRASTRUCTURE ONLY): the design and the update of pss_exec.h — the code the
// kernels of spicey_amd/csrc/pss.hip run — through an emulation of their mapping: one "thread" per (instance, state entry) runs
// spicey_pss_design; per circuit an emulated workgroup of `threads` threads runs spicey_pss_update, every phase in all its
// threads in turn (the highest first: nothing may depend on the order) with the barrier behind it, the pivot search in 64 lanes
// met at stride 32 .. 1 as the device's first wave meets them.  The calls are judged by spicey_pss_judge of pss.h, the judge of
// the library's entry points, and run on a workspace laid out as the launchers lay out the device's.  Compiled with
// -ffp-contract=off like the kernels' translation unit, so the results are the GPU's bit for bit.
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/pss.h"

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
  void pivot(const double *M, int32_t nX, int32_t k, SpiceyPssShared *sh) {
    SpiceyPssPiv p[SPICEY_PSS_LANES];
    for (int32_t l = SPICEY_PSS_LANES - 1; l >= 0; l--) p[l] = spicey_pss_piv_lane(M, nX, k, l);
    for (int stride = SPICEY_PSS_LANES / 2; stride > 0; stride >>= 1)
      for (int l = 0; l < stride; l++) spicey_pss_piv_meet(&p[l], p[l + stride]);
    spicey_pss_piv_done(sh, k, p[0]);
  }
};
}  // namespace

extern "C" int64_t spicey_pss_host_workspace_bytes(int32_t n_ckt, int32_t nX, int32_t method) { return spicey_pss_bytes(n_ckt, nX, method); }
extern "C" int32_t spicey_pss_host_req_bytes(void) { return (int32_t)sizeof(SpiceyPssReq); }
extern "C" int64_t spicey_pss_host_lds_bytes(int32_t method, int32_t nX) { return (int64_t)spicey_pss_lds_bytes(method, nX); }

// have_work = 0 stands for a null workspace, work_bytes = -1 for a workspace of exactly the size needed.  Returns SPICEY_OK or
// SPICEY_ERR_BAD_DESC (text in err; the results untouched).
extern "C" int32_t spicey_pss_host_design(int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, int32_t perturb, const double *base,
                                          const int32_t *base_on, double *h, double *Cv, double *Li, double *Dv, int32_t *Son, int32_t have_work, int64_t work_bytes,
                                          char *err, int32_t err_cap) {
  std::string e;
  SpiceyPssArgs A;
  if (!spicey_pss_judge(false, nC, nL, nD, nS, req, perturb, (double *)base, (int32_t *)base_on, h, Cv, Li, Dv, Son, nullptr, nullptr, nullptr, have_work != 0,
                        work_bytes < 0 ? INT64_MAX : work_bytes, A, e))
    return refuse(e, err, err_cap);
  SpiceyPssLayout l{};
  spicey_pss_layout(A.n_ckt, spicey_pss_nx(A), A.method, l);
  std::vector<char> work((size_t)l.total_bytes);
  spicey_pss_head(l, A, nullptr, work.data(), work.data());
  const int64_t total = l.n_inst * spicey_pss_nx(A);
  for (int64_t idx = 0; idx < total; idx++) spicey_pss_design(A, idx);
  return SPICEY_OK;
}

// threads: the emulated workgroup (0: 256).
extern "C" int32_t spicey_pss_host_update(int32_t nC, int32_t nL, int32_t nD, int32_t nS, const SpiceyPssReq *req, const int32_t *ist, double *base, int32_t *base_on,
                                          const double *h, const double *Cv, const double *Li, const double *Dv, const int32_t *Son, double *delta, double *rows,
                                          int32_t *done, int32_t have_work, int64_t work_bytes, int32_t threads, char *err, int32_t err_cap) {
  std::string e;
  SpiceyPssArgs A;
  if (!spicey_pss_judge(true, nC, nL, nD, nS, req, 1, base, base_on, (double *)h, (double *)Cv, (double *)Li, (double *)Dv, (int32_t *)Son, delta, rows, done,
                        have_work != 0, work_bytes < 0 ? INT64_MAX : work_bytes, A, e))
    return refuse(e, err, err_cap);
  SpiceyPssLayout l{};
  spicey_pss_layout(A.n_ckt, spicey_pss_nx(A), A.method, l);
  std::vector<char> work((size_t)l.total_bytes);
  spicey_pss_head(l, A, ist, work.data(), work.data());
  // (the matrix: exactly the bytes of the device's dynamic LDS, so a sanitizer sees an access past them)
  std::vector<double> M(spicey_pss_lds_bytes(A.method, spicey_pss_nx(A)) / sizeof(double));
  HostWorkgroup wg{threads > 0 ? threads : SPICEY_PSS_THREADS};
  for (int32_t c = 0; c < A.n_ckt; c++) {
    SpiceyPssShared sh;
    memset(&sh, 0x5a, sizeof(sh));  // (LDS is not cleared between workgroups)
    spicey_pss_update(A, c, M.data(), &sh, wg);
  }
  return SPICEY_OK;
}
