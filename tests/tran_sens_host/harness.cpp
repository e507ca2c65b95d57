// CPU harness of the sensitivities and corners of transient measurements (TEST INFRASTRUCTURE ONLY): the design and the
// reduction of tran_sens_exec.h — the code the kernels of spicey_amd/csrc/tran_sens.hip run — through an emulation of their
// mapping: one "thread" per (instance, element) runs spicey_ts_design; per scalar `threads` / 64 waves are emulated of which the
// first, as on the device, runs spicey_ts_lane in its 64 lanes and meets them by spicey_ts_meet at stride 32 .. 1 (the thread
// count changes the order in which lanes are visited, nothing else: nothing may depend on it).  The scalars are spicey_tmc_scalar
// of tran_mc_exec.h.  The calls are judged by spicey_ts_design_judge / spicey_ts_reduce_judge of tran_sens.h, the judges of the
// library's entry points, and run on workspaces laid out as the launchers lay out the device's.  Compiled with
// -ffp-contract=off like the kernels' translation unit, so the results are the GPU's bit for bit.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/tran_sens.h"

namespace {
int32_t refuse(const std::string &e, char *err, int32_t err_cap) {
  if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
  return SPICEY_ERR_BAD_DESC;
}
}  // namespace

extern "C" int64_t spicey_ts_host_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t nA) { return spicey_ts_workspace_bytes(n_inst, n_scalar, nE, nA); }
extern "C" int32_t spicey_ts_host_req_bytes(void) { return (int32_t)sizeof(SpiceyTranSensReq); }

// have_work = 0 stands for a null workspace, work_bytes = -1 for a workspace of exactly the size needed.  Returns SPICEY_OK or
// SPICEY_ERR_BAD_DESC (text in err; the results untouched).
extern "C" int32_t spicey_ts_host_design(int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *R, const double *Cv, const double *Lv,
                                         const SpiceyTranSensReq *req, const int32_t *act, const double *step, const int8_t *lvl, const double *tol, double *oR, double *oC,
                                         double *oL, int32_t have_work, int64_t work_bytes, char *err, int32_t err_cap) {
  std::string e;
  SpiceyTsDesignArgs A;
  if (!spicey_ts_design_judge(n_inst, nR, nC, nL, R, Cv, Lv, req, -1, act, step, lvl, tol, oR, oC, oL, have_work != 0, work_bytes < 0 ? INT64_MAX : work_bytes, A, e))
    return refuse(e, err, err_cap);
  SpiceyTsDesignLayout l{};
  spicey_ts_design_layout(A.mode, n_inst, nR + nC + nL, A.nA, l);
  std::vector<char> work((size_t)l.total_bytes);
  spicey_ts_design_head(l, A, act, step, lvl, tol, work.data(), work.data());
  const int64_t total = (int64_t)n_inst * ((int64_t)nR + nC + nL);
  for (int64_t idx = 0; idx < total; idx++) spicey_ts_design(A, idx);
  return SPICEY_OK;
}

// threads: a multiple of 64, the emulated workgroup (0: 64).  have_out = 0 stands for null result buffers, work_bytes = -1 for a
// workspace of exactly the size needed.  rows [3] hold HOST pointers here.
extern "C" int32_t spicey_ts_host_reduce(int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar, const uint8_t *valid,
                                         const double *step, const double *tol_act, int32_t nA, double *x, double *sens, int8_t *sign, double *bound, int32_t have_out,
                                         int64_t work_bytes, int32_t threads, char *err, int32_t err_cap) {
  std::string e;
  SpiceyTmcArgs T;
  SpiceyTsReduceArgs A;
  if (!spicey_ts_reduce_judge(n_inst, rows, scalars, n_scalar, step, tol_act, nA, have_out != 0 && x && sens && sign && bound, work_bytes < 0 ? INT64_MAX : work_bytes, T, A, e))
    return refuse(e, err, err_cap);
  SpiceyTsReduceLayout l{};
  spicey_ts_reduce_layout(n_inst, n_scalar, nA, l);
  std::vector<char> work((size_t)l.total_bytes);
  spicey_tmc_head(l.tmc, T, scalars, valid, nullptr, nullptr, nullptr, x, work.data(), work.data());
  spicey_ts_reduce_head(l, A, valid, step, tol_act, x, sens, sign, bound, work.data() + l.off_rec, work.data());
  for (int64_t idx = 0; idx < (int64_t)n_inst * n_scalar; idx++) spicey_tmc_scalar(T, idx);
  const int32_t waves = threads > SPICEY_MC_LANES ? threads / SPICEY_MC_LANES : 1;
  for (int32_t j = 0; j < n_scalar; j++) {
    SpiceyTsPartial p[SPICEY_MC_LANES];
    // (the waves of a larger workgroup take the lanes in turn, the highest wave first: lane l's work is the same wherever it runs)
    for (int32_t w = waves - 1; w >= 0; w--)
      for (int32_t l2 = w; l2 < SPICEY_MC_LANES; l2 += waves) spicey_ts_lane(A, j, l2, &p[l2]);
    for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1)
      for (int l2 = 0; l2 < stride; l2++) spicey_ts_meet(&p[l2], p[l2 + stride]);
    spicey_ts_bound_row(A, j, p[0]);
  }
  return SPICEY_OK;
}
