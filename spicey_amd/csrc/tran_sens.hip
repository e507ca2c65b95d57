// tran_sens.hip — sensitivities and corners of transient measurements on the device (spicey_tran_sens_design_device,
// spicey_tran_sens_reduce_device, spicey_run_sens, spicey_run_levels): kernels and launchers.
//
// tran_sens_exec.h holds the arithmetic, the mapping and the summation order, shared with the CPU harness of
// tests/tran_sens_host.  Two kernels, no atomics, nothing waits for another workgroup:
//   design   one thread per (instance, element): one or two loads, one product, one store.
//   reduce   one wave per scalar: lane l reads x0 and, per element a = l, l + 64, ..., the two perturbed values — a column of
//            x, stride n_scalar doubles, a few hundred values at most —, writes the element's {d, c} and sign and keeps its
//            partial sums in registers; the lanes meet by __shfl_down, stride 32 .. 1, and lane 0 writes the bound row.  No
//            LDS.  A wave, not a workgroup: nA is the toleranced elements of one circuit, tens to a few hundred.
// The scalars in between are tran_mc.hip's kernel (spicey_launch_tmc_scalars).
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit (as tran_mc.hip); f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "devbuf.h"
#include "measure.h"
#include "tran_sens.h"

namespace {

static_assert(SPICEY_MC_LANES == 64, "the reducing wave: gfx950 waves have 64 lanes");

__global__ void __launch_bounds__(SPICEY_MC_THREADS) spicey_ts_design_kernel(const SpiceyTsDesignArgs *__restrict__ Ap, int64_t total_threads) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MC_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceyTsDesignArgs A = *Ap;
  spicey_ts_design(A, idx);
}

__device__ __forceinline__ SpiceyTsPartial ts_shfl_down(const SpiceyTsPartial &p, int stride) {
  SpiceyTsPartial q;
  q.wc = __shfl_down(p.wc, stride);
  q.rss2 = __shfl_down(p.rss2, stride);
  q.m = __shfl_down(p.m, stride);
  q.n_num = __shfl_down(p.n_num, stride);
  q.n_int = __shfl_down(p.n_int, stride);
  q.a = __shfl_down(p.a, stride);
  return q;
}

__global__ void __launch_bounds__(SPICEY_MC_LANES) spicey_ts_reduce_kernel(const SpiceyTsReduceArgs *__restrict__ Ap) {
  const SpiceyTsReduceArgs A = *Ap;
  const int32_t j = (int32_t)blockIdx.x, lane = (int32_t)threadIdx.x;
  if (j >= A.n_scalar) return;  // (the whole wave: no lane is missing from the shuffles below)
  SpiceyTsPartial p;
  spicey_ts_lane(A, j, lane, &p);
  // p[l] meets p[l + stride] for l < stride; the lanes above take what no later stride reads
  for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1) spicey_ts_meet(&p, ts_shfl_down(p, stride));
  if (lane == 0) spicey_ts_bound_row(A, j, p);
}

}  // namespace

hipError_t spicey_launch_ts_design(int device, const SpiceyTsDesignArgs &A0, const int32_t *act, const double *step, const int8_t *lvl, const double *tol, void *d_work,
                                   hipStream_t st) {
  hipError_t e;
  const int64_t nE = (int64_t)A0.nR + A0.nC + A0.nL;
  SpiceyTsDesignLayout l;
  if (!spicey_ts_design_layout(A0.mode, A0.n_inst, (int32_t)nE, A0.nA, l)) return hipErrorInvalidValue;
  // (the record and its arrays in one copy: the record names their places behind it)
  SpiceyTsDesignArgs A = A0;
  std::vector<char> head((size_t)l.total_bytes);
  spicey_ts_design_head(l, A, act, step, lvl, tol, head.data(), (char *)d_work);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const int64_t total = (int64_t)A.n_inst * nE;
  unsigned grid = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MC_THREADS, &grid)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_ts_design_kernel, dim3(grid), dim3(SPICEY_MC_THREADS), 0, st, (const SpiceyTsDesignArgs *)d_work, total);
  return hipGetLastError();
}

hipError_t spicey_launch_ts_reduce(int device, const SpiceyTmcArgs &T, const SpiceyTsReduceArgs &A0, const SpiceyMcScalar *scalars, const uint8_t *valid,
                                   const double *step, const double *tol_act, double *d_x, double *d_sens, int8_t *d_sign, double *d_bound, void *d_work, hipStream_t st) {
  hipError_t e;
  SpiceyTsReduceLayout l;
  if (!spicey_ts_reduce_layout(A0.n_inst, A0.n_scalar, A0.nA, l) || (int64_t)A0.n_inst != 1 + 2 * (int64_t)A0.nA) return hipErrorInvalidValue;
  if ((e = spicey_launch_tmc_scalars(device, T, scalars, valid, nullptr, nullptr, nullptr, d_x, d_work, st)) != hipSuccess) return e;
  SpiceyTsReduceArgs A = A0;
  std::vector<char> head((size_t)(l.total_bytes - l.off_rec));
  spicey_ts_reduce_head(l, A, valid, step, tol_act, d_x, d_sens, d_sign, d_bound, head.data(), (char *)d_work);
  if ((e = spicey_upload_table_async(device, (char *)d_work + l.off_rec, head.data(), head.size(), st)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_ts_reduce_kernel, dim3((unsigned)A.n_scalar), dim3(SPICEY_MC_LANES), 0, st, (const SpiceyTsReduceArgs *)((const char *)d_work + l.off_rec));
  return hipGetLastError();
}
