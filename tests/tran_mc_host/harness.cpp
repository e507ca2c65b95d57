// CPU harness of the Monte Carlo of transient runs (TEST INFRASTRUCTURE ONLY): the draw, the scalar programs and the reduction
// of tran_mc_exec.h — the code the kernels of spicey_amd/csrc/tran_mc.hip run — through an emulation of their mapping: one
// "thread" per (sample, element) runs spicey_tmc_draw, one per (sample, scalar) spicey_tmc_scalar, one per sample
// spicey_tmc_sample; per scalar a workgroup of `threads` threads loads and sorts the keys (par = a loop over t), every thread's
// binary searches are done once, 64 lanes run spicey_tmc_stat_lane and meet by spicey_tmc_stat_meet at stride 32 .. 1, and every
// thread writes its order statistics.  The calls are judged by spicey_tmc_draw_judge / spicey_tmc_reduce_judge of tran_mc.h, the
// judges of the library's entry points, and the reduction runs on a workspace laid out by spicey_tmc_layout / spicey_tmc_head
// as the launcher lays out the device's.  Compiled with -ffp-contract=off like the kernels' translation unit, so the results are
// the GPU's bit for bit.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/tran_mc.h"

namespace {
int32_t refuse(const std::string &e, char *err, int32_t err_cap) {
  if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
  return SPICEY_ERR_BAD_DESC;
}
}  // namespace

extern "C" int64_t spicey_tmc_host_workspace_bytes(int32_t n_inst, int32_t n_scalar, int32_t nE, int32_t log2K, int32_t n_prob) {
  return spicey_tmc_workspace_bytes(n_inst, n_scalar, nE, log2K, n_prob);
}
extern "C" int32_t spicey_tmc_host_req_bytes(void) { return (int32_t)sizeof(SpiceyTranMcReq); }
extern "C" int32_t spicey_tmc_host_scalar_bytes(void) { return (int32_t)sizeof(SpiceyMcScalar); }

extern "C" void spicey_tmc_host_keys(const double *x, int64_t n, uint64_t *keys, double *back) {
  for (int64_t i = 0; i < n; i++) {
    keys[i] = spicey_tmc_key(x[i]);
    back[i] = spicey_tmc_unkey(keys[i]);
  }
}

// have_work = 0 stands for a null workspace, work_bytes = -1 for a workspace of exactly the size needed.  Returns SPICEY_OK or
// SPICEY_ERR_BAD_DESC (text in err; the results untouched).
extern "C" int32_t spicey_tmc_host_draw(int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *R, const double *Cv, const double *Lv, const double *tol,
                                        const double *icdf, const SpiceyTranMcReq *req, double *oR, double *oC, double *oL, int32_t have_work, int64_t work_bytes,
                                        char *err, int32_t err_cap) {
  std::string e;
  SpiceyMcDrawArgs A;
  const int64_t need = req ? spicey_mc_draw_bytes(nR + nC + nL, req->log2K) : 0;
  if (!spicey_tmc_draw_judge(n_inst, nR, nC, nL, R, Cv, Lv, tol, icdf, req, oR, oC, oL, have_work != 0, work_bytes < 0 ? need : work_bytes, A, e))
    return refuse(e, err, err_cap);
  A.tol = tol;
  A.icdf = icdf;
  const int64_t total = (int64_t)n_inst * ((int64_t)nR + nC + nL);
  for (int64_t idx = 0; idx < total; idx++) spicey_tmc_draw(A, idx);
  return SPICEY_OK;
}

// threads = 0: the launcher's choice.  have_out = 0 stands for null result buffers, work_bytes = -1 for a workspace of exactly
// the size needed.  rows [3] hold HOST pointers here.
extern "C" int32_t spicey_tmc_host_reduce(int32_t n_inst, const SpiceyMcRows *rows, const SpiceyMcScalar *scalars, int32_t n_scalar, const uint8_t *valid,
                                          const double *lo, const double *hi, const double *probs, int32_t n_prob, double *x, double *stat, int64_t *sample,
                                          int32_t have_out, int64_t work_bytes, int32_t threads, char *err, int32_t err_cap) {
  std::string e;
  SpiceyTmcArgs A;
  const int64_t need = spicey_tmc_reduce_bytes(n_inst, n_scalar, n_prob);
  if (!spicey_tmc_reduce_judge(n_inst, rows, scalars, n_scalar, lo, hi, probs, n_prob, have_out != 0 && x && stat && sample, work_bytes < 0 ? need : work_bytes, A, e))
    return refuse(e, err, err_cap);
  SpiceyTmcLayout l{};
  spicey_tmc_layout(n_inst, n_scalar, n_prob, l);
  std::vector<char> work((size_t)l.total_bytes);
  spicey_tmc_head(l, A, scalars, valid, lo, hi, probs, x, work.data(), work.data());
  if (threads > 0) A.sort_threads = threads;
  for (int64_t idx = 0; idx < (int64_t)n_inst * n_scalar; idx++) spicey_tmc_scalar(A, idx);
  for (int64_t s = 0; s < n_inst; s++) spicey_tmc_sample(A, s, sample);
  std::vector<uint64_t> keys((size_t)A.n_pad);
  const int32_t T = A.sort_threads;
  const auto par = [T](auto f) {
    for (int32_t t = 0; t < T; t++) f(t);
  };
  for (int32_t j = 0; j < n_scalar; j++) {
    for (int32_t t = 0; t < T; t++)
      for (int32_t i = t; i < A.n_pad; i += T) keys[(size_t)i] = spicey_tmc_key_of(A, i, j);
    spicey_mc_sort(par, T, keys.data(), A.n_pad);
    const int32_t n_num = spicey_tmc_count_below(keys.data(), A.n_pad, SPICEY_TMC_NAN_KEY);
    const int32_t n_valid = spicey_tmc_count_below(keys.data(), A.n_pad, SPICEY_MC_PAD_KEY);
    SpiceyTmcPartial p[SPICEY_MC_LANES];
    for (int l2 = 0; l2 < SPICEY_MC_LANES; l2++) spicey_tmc_stat_lane(A, j, keys.data(), n_valid, n_num, l2, &p[l2]);
    for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1)
      for (int l2 = 0; l2 < stride; l2++) spicey_tmc_stat_meet(&p[l2], p[l2 + stride]);
    spicey_tmc_stat_row(A, j, n_valid, n_num, p[0], stat);
    for (int32_t t = 0; t < T; t++) spicey_tmc_stat_ranks(A, j, keys.data(), n_num, t, T, stat);
  }
  return SPICEY_OK;
}
