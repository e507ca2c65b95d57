// CPU harness of the Monte Carlo tolerance analysis (TEST INFRASTRUCTURE ONLY): the draw and the reduction of mc_exec.h — the
// code the kernels of spicey_amd/csrc/mc.hip run — through an emulation of their mapping: one "thread" per (sample, element)
// runs spicey_mc_draw; per sample s < n_pad 64 lanes run spicey_mc_sample_lane and meet by spicey_mc_sample_meet at stride 32 .. 1;
// per frequency a workgroup of `threads` threads sorts the row of keys (par = a loop over t), 64 lanes run spicey_mc_freq_lane,
// their partials meet by s[l] += s[l + stride], and every thread writes its order statistics.  The calls are judged by
// spicey_mc_draw_judge / spicey_mc_reduce_judge of mc.h, the judges of the library's entry points, and the reduction runs on a
// workspace laid out by spicey_mc_layout / spicey_mc_reduce_head as the launcher lays out the device's.  Compiled with
// -ffp-contract=off like the kernels' translation unit, so the results are the GPU's bit for bit.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/mc.h"

namespace {
int32_t refuse(const std::string &e, char *err, int32_t err_cap) {
  if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
  return SPICEY_ERR_BAD_DESC;
}
}  // namespace

extern "C" int64_t spicey_mc_host_workspace_bytes(int32_t n_inst, int64_t n_freq, int32_t nE, int32_t log2K, int32_t n_rank) {
  return spicey_mc_workspace_bytes(n_inst, n_freq, nE, log2K, n_rank);
}
extern "C" int32_t spicey_mc_host_req_bytes(void) { return (int32_t)sizeof(SpiceyAcMcReq); }

extern "C" void spicey_mc_host_philox(uint32_t *c, uint32_t k0, uint32_t k1) { spicey_mc_philox(c, k0, k1); }

// m [n_inst][nE]: the 52 uniform bits of every (sample, element)
extern "C" void spicey_mc_host_uniform(uint64_t seed, int32_t n_inst, int32_t nE, uint64_t *m) {
  for (int32_t s = 0; s < n_inst; s++)
    for (int32_t e = 0; e < nE; e++) m[(int64_t)s * nE + e] = spicey_mc_uniform(seed, (uint32_t)s, (uint32_t)e);
}

// have_work = 0 stands for a null workspace, work_bytes = -1 for a workspace of exactly the size needed.  Returns SPICEY_OK or
// SPICEY_ERR_BAD_DESC (text in err; the results untouched).
extern "C" int32_t spicey_mc_host_draw(int32_t n_inst, int32_t nR, int32_t nC, int32_t nL, const double *R, const double *Cv, const double *Lv, const double *tol,
                                       const double *icdf, const SpiceyAcMcReq *req, double *oR, double *oC, double *oL, int32_t have_work, int64_t work_bytes,
                                       char *err, int32_t err_cap) {
  std::string e;
  SpiceyMcDrawArgs A;
  const int64_t need = req ? spicey_mc_draw_bytes(nR + nC + nL, req->log2K) : 0;
  if (!spicey_mc_draw_judge(n_inst, nR, nC, nL, R, Cv, Lv, tol, icdf, req, oR, oC, oL, have_work != 0, work_bytes < 0 ? need : work_bytes, A, e))
    return refuse(e, err, err_cap);
  A.tol = tol;
  A.icdf = icdf;
  const int64_t total = (int64_t)n_inst * ((int64_t)nR + nC + nL);
  for (int64_t idx = 0; idx < total; idx++) spicey_mc_draw(A, idx);
  return SPICEY_OK;
}

// The keys x [n_pad] sorted as a workgroup of `threads` threads sorts them.
extern "C" void spicey_mc_host_sort(uint64_t *x, int32_t n_pad, int32_t threads) {
  const auto par = [threads](auto f) {
    for (int32_t t = 0; t < threads; t++) f(t);
  };
  spicey_mc_sort(par, threads, x, n_pad);
}

// threads = 0: the launcher's choice.  have_out = 0 stands for null result buffers, work_bytes = -1 for a workspace of exactly
// the size needed.
extern "C" int32_t spicey_mc_host_reduce(int32_t n_inst, int64_t n_freq, const double *v, int32_t n_v, const uint8_t *valid, const double *lo, const double *hi,
                                         const int64_t *ranks, int32_t n_rank, const SpiceyAcMcReq *req, int64_t *sample, double *freq, int32_t have_out,
                                         int64_t work_bytes, int32_t threads, char *err, int32_t err_cap) {
  std::string e;
  SpiceyMcReduceArgs A;
  const int64_t need = spicey_mc_reduce_bytes(n_inst, n_freq, n_rank);
  if (!spicey_mc_reduce_judge(n_inst, n_freq, v, n_v, valid, ranks, n_rank, req, have_out != 0 && sample && freq, work_bytes < 0 ? need : work_bytes, A, e))
    return refuse(e, err, err_cap);
  SpiceyMcLayout l{};
  spicey_mc_layout(n_inst, n_freq, n_rank, l);
  std::vector<char> work((size_t)l.total_bytes);
  spicey_mc_reduce_head(l, A, valid, lo, hi, ranks, work.data(), work.data());
  if (threads > 0) A.sort_threads = threads;
  for (int64_t s = 0; s < A.n_pad; s++) {
    int64_t count[SPICEY_MC_LANES], first[SPICEY_MC_LANES];
    for (int l2 = 0; l2 < SPICEY_MC_LANES; l2++) spicey_mc_sample_lane(A, s, l2, &count[l2], &first[l2]);
    for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1)
      for (int l2 = 0; l2 < stride; l2++) spicey_mc_sample_meet(&count[l2], &first[l2], count[l2 + stride], first[l2 + stride]);
    spicey_mc_sample_row(A, s, count[0], first[0], sample);
  }
  std::vector<uint64_t> keys((size_t)A.n_pad);
  const int32_t T = A.sort_threads;
  for (int64_t k = 0; k < n_freq; k++) {
    memcpy(keys.data(), A.qT + k * A.n_pad, (size_t)A.n_pad * sizeof(uint64_t));
    spicey_mc_host_sort(keys.data(), A.n_pad, T);
    double s[SPICEY_MC_LANES][2];
    int64_t viol[SPICEY_MC_LANES];
    for (int l2 = 0; l2 < SPICEY_MC_LANES; l2++) spicey_mc_freq_lane(A, k, keys.data(), l2, s[l2], &viol[l2]);
    for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1)
      for (int l2 = 0; l2 < stride; l2++) {
        s[l2][0] = s[l2][0] + s[l2 + stride][0];
        s[l2][1] = s[l2][1] + s[l2 + stride][1];
        viol[l2] += viol[l2 + stride];
      }
    spicey_mc_freq_row(A, k, s[0], viol[0], freq);
    for (int32_t t = 0; t < T; t++) spicey_mc_freq_ranks(A, k, keys.data(), t, T, freq);
  }
  return SPICEY_OK;
}
