// ac_measure.hip — device-side measurements over an AC sweep (spicey_ac_measure_device, spicey_ac_run_measure): kernel and
// launcher.
//
// A reduction pass over the complex buffers [inst][freq][col][2] a sweep wrote; ac_measure_exec.h holds the arithmetic, the
// mapping and its reasons, shared with the CPU harness of tests/ac_measure_host.  One kernel: a wave per (instance,
// request) pair — the table is sorted by column, so the waves of a workgroup read neighbouring columns of the same rows —
// whose lanes stride over the window, meet in a butterfly of cross-lane moves and leave the row to lane 0.  No LDS, no
// atomics, no barrier, nothing waits for another workgroup.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit (as measure.hip); f64 division is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup
// sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "ac_measure.h"
#include "ac_measure_exec.h"
#include "measure.h"

namespace {

static_assert(SPICEY_ACM_LANES == 64, "one pair per wave: gfx950 waves have 64 lanes");

__global__ void __launch_bounds__(SPICEY_ACM_THREADS) spicey_ac_measure_kernel(SpiceyAcmBufs B, int64_t total, const SpiceyAcMeasDevReq *__restrict__ table,
                                                                              int32_t n_req, double *__restrict__ meas) {
  const int lane = (int)(threadIdx.x & (SPICEY_ACM_LANES - 1));
  // (the wave's number is the same in all its lanes: as a scalar, so are the pair and its request record)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SPICEY_ACM_LANES));
  const int per_wg = SPICEY_ACM_THREADS / SPICEY_ACM_LANES;
  for (int64_t idx = (int64_t)blockIdx.x * per_wg + wave; idx < total; idx += (int64_t)gridDim.x * per_wg) {
    const int64_t inst = idx / n_req;
    const SpiceyAcMeasDevReq q = table[idx - inst * n_req];
    const double thr = spicey_acm_thr(B, q, inst);
    SpiceyAcmPart p = spicey_acm_lane(B, q, inst, lane, SPICEY_ACM_LANES, thr);
    for (int off = SPICEY_ACM_LANES / 2; off > 0; off >>= 1) {
      SpiceyAcmPart o;
      o.v0 = __shfl_xor(p.v0, off);
      o.v1 = __shfl_xor(p.v1, off);
      o.k0 = __shfl_xor((long long)p.k0, off);
      o.k1 = __shfl_xor((long long)p.k1, off);
      o.cnt = __shfl_xor((long long)p.cnt, off);
      spicey_acm_combine(q.kind, p, o);
    }
    if (lane == 0) {
      double out[8];
      spicey_acm_finish(B, q, inst, p, thr, out);
      double *dst = meas + (inst * n_req + q.orig) * 8;
      for (int j = 0; j < 8; j++) dst[j] = out[j];
    }
  }
}

}  // namespace

hipError_t spicey_launch_ac_measure(int device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                    const SpiceyAcMeasDevReq *table, int32_t n_req, double *d_meas, void *d_work, hipStream_t st) {
  const hipError_t e = spicey_upload_table_async(device, d_work, table, (size_t)n_req * sizeof(SpiceyAcMeasDevReq), st);
  if (e != hipSuccess) return e;
  const SpiceyAcmBufs B{d_v, d_i, n_v, n_i, n_freq};
  const int64_t total = (int64_t)n_inst * n_req, per_wg = SPICEY_ACM_THREADS / SPICEY_ACM_LANES;
  // (one wave per pair; beyond the grid's cap a wave takes several pairs)
  hipLaunchKernelGGL(spicey_ac_measure_kernel, dim3(spicey_meas_grid1((total + per_wg - 1) / per_wg)), dim3(SPICEY_ACM_THREADS), 0, st, B, total,
                     (const SpiceyAcMeasDevReq *)d_work, n_req, d_meas);
  return hipGetLastError();
}
