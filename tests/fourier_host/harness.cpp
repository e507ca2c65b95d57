// CPU harness of the harmonics pass: fourier_exec.h — the code the kernels of spicey_amd/csrc/fourier.hip run — through an
// emulation of their lane, tile and chunk mapping: workgroups of `threads` threads take the stage 1 tiles blockIdx,
// blockIdx + grid, ..., every thread of a workgroup does what spicey_four_stage1 gives it (lane = t % rl, slot = t / rl),
// then one thread per (instance, request, row element) combines (spicey_four_stage2).  The twiddle table is the one the
// library uploads (spicey_four_head).  Compiled with -ffp-contract=off like the kernels' translation unit, so the results
// are the GPU's bit for bit.  The partials start as NaNs: one that is read without having been written shows.
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../spicey_amd/csrc/fourier_exec.h"

extern "C" int32_t spicey_four_host_chunk(void) { return SPICEY_MEAS_CHUNK; }
extern "C" int32_t spicey_four_host_threads(void) { return SPICEY_MEAS_THREADS; }
extern "C" int32_t spicey_four_host_max_harm(void) { return SPICEY_FOUR_MAX_HARM; }
extern "C" int64_t spicey_four_host_workspace_bytes(int32_t n_inst, int64_t n_points, const SpiceyFourReq *reqs, int32_t n_req) {
  return spicey_four_workspace_bytes(n_inst, n_points, reqs, n_req);
}
extern "C" void spicey_four_host_twiddle(int32_t h, int64_t s, double f0dt, double *cs) { spicey_four_twiddle(h, s, f0dt, cs, cs + 1); }

// threads: a power of two, 1 .. 1024; grid: workgroups launched, 0 = one per tile; work_bytes: what the caller claims its
// workspace holds (-1: exactly enough).  Returns SPICEY_OK or SPICEY_ERR_BAD_DESC (text in err; `out` untouched).
extern "C" int32_t spicey_four_host_run(int32_t n_inst, int64_t n_points, double dt, const double *v, int32_t n_v, const double *i, int32_t n_i,
                                        const SpiceyFourReq *reqs, int32_t n_req, double *out, int32_t out_stride, int64_t work_bytes, int32_t threads,
                                        int64_t grid, char *err, int32_t err_cap) {
  std::string e;
  SpiceyFourPlan p;
  bool ok = threads >= 1 && threads <= 1024 && (threads & (threads - 1)) == 0 && grid >= 0;
  if (!ok) e = "fourier: bad arguments";
  ok = ok && spicey_four_judge(n_inst, n_points, dt, v != nullptr, n_v, i != nullptr, n_i, reqs, n_req, out != nullptr, out_stride,
                               work_bytes < 0 ? std::numeric_limits<int64_t>::max() : work_bytes, p, e);
  if (!ok) {
    if (err && err_cap > 0) { strncpy(err, e.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return SPICEY_ERR_BAD_DESC;
  }
  std::vector<unsigned char> head;
  spicey_four_head(p, dt, head);
  spicey_four_geom(p, threads);  // (the tiles of the emulated workgroup size; the head's copy of the bases is not used below)
  const SpiceyFourDevReq *table = p.table.data();
  const double *tw = (const double *)(head.data() + p.off_tw);
  std::vector<double> partials((size_t)((int64_t)n_inst * p.partials_per_inst), std::numeric_limits<double>::quiet_NaN());
  const int64_t tiles = (int64_t)n_inst * p.tiles_per_inst;
  const int64_t blocks = grid == 0 || grid > tiles ? tiles : grid;
  for (int64_t b = 0; b < blocks; b++)
    for (int64_t tile = b; tile < tiles; tile += blocks)
      for (int32_t t = 0; t < threads; t++)
        spicey_four_stage1(tile, t % p.rl, t / p.rl, p.rl, p.cl, p.tiles_per_inst, table, p.bases.data(), (int32_t)p.bases.size(), tw, n_points, v, n_v, i, n_i,
                           partials.data(), p.partials_per_inst);
  for (int64_t idx = 0; idx < (int64_t)n_inst * n_req * out_stride; idx++)
    spicey_four_stage2(idx, table, p.bases.data(), n_req, out_stride, partials.data(), p.partials_per_inst, out);
  return SPICEY_OK;
}
