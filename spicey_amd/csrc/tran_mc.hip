// tran_mc.hip — Monte Carlo of transient runs on the device (spicey_tran_mc_draw_device, spicey_tran_mc_reduce_device,
// spicey_run_mc): kernels and launchers.
//
// tran_mc_exec.h holds the arithmetic, the mapping and the summation order, shared with the CPU harness of tests/tran_mc_host.
// Four kernels, no atomics, nothing waits for another workgroup:
//   draw     one thread per (sample, element), as mc.hip's, the resistor left in ohms.
//   scalar   one thread per (scalar, sample), the sample the fast index: a wave runs ONE program on 64 neighbouring samples, so
//            it does not diverge on the opcodes and fetches the program's record once; a few loads and at most 48 operations.
//   sample   one thread per sample over its n_scalar values of x.  A thread, not a wave: n_scalar is a handful to a few dozen
//            consecutive doubles, which a wave's 64 lanes would mostly idle over, and the thread's loop keeps "the lowest
//            violated j" free of any cross-lane step.
//   stat     one workgroup per scalar: the column's n_pad keys into dynamic LDS (8 n_pad bytes, 128 KiB at 16384 samples: one
//            workgroup per CU there), the bitonic network of mc_exec.h on them as unsigned integers, a barrier between stages;
//            every thread finds n_valid and n_num by binary search in the sorted keys; wave 0 forms the two sums in the fixed
//            lane order, the violations and the extreme samples, its lanes meeting by __shfl_down; every thread writes its share
//            of the order statistics.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit (as mc.hip); f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "devbuf.h"
#include "measure.h"
#include "tran_mc.h"

namespace {

static_assert(SPICEY_MC_LANES == 64, "the summing wave: gfx950 waves have 64 lanes");

__global__ void __launch_bounds__(SPICEY_MC_THREADS) spicey_tmc_draw_kernel(const SpiceyMcDrawArgs *__restrict__ Ap, int64_t total_threads) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MC_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceyMcDrawArgs A = *Ap;
  spicey_tmc_draw(A, idx);
}

__global__ void __launch_bounds__(SPICEY_MC_THREADS) spicey_tmc_scalar_kernel(const SpiceyTmcArgs *__restrict__ Ap, int64_t total_threads) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MC_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  spicey_tmc_scalar(*Ap, idx);  // (the record where it lies: a FIELD's pass indexes it)
}

__global__ void __launch_bounds__(SPICEY_MC_THREADS) spicey_tmc_sample_kernel(const SpiceyTmcArgs *__restrict__ Ap, int64_t *__restrict__ sample) {
  const int64_t s = (int64_t)blockIdx.x * SPICEY_MC_THREADS + threadIdx.x;
  const SpiceyTmcArgs A = *Ap;
  if (s >= A.n_inst) return;
  spicey_tmc_sample(A, s, sample);
}

__device__ __forceinline__ SpiceyTmcPartial tmc_shfl_down(const SpiceyTmcPartial &p, int stride) {
  SpiceyTmcPartial q;
  q.s0 = __shfl_down(p.s0, stride);
  q.s1 = __shfl_down(p.s1, stride);
  q.viol = __shfl_down((long long)p.viol, stride);
  q.s_min = __shfl_down((long long)p.s_min, stride);
  q.s_max = __shfl_down((long long)p.s_max, stride);
  return q;
}

__global__ void __launch_bounds__(SPICEY_MC_SORT_MAX) spicey_tmc_stat_kernel(const SpiceyTmcArgs *__restrict__ Ap, double *__restrict__ stat) {
  extern __shared__ uint64_t keys[];
  const SpiceyTmcArgs A = *Ap;
  const int32_t t = (int32_t)threadIdx.x, T = (int32_t)blockDim.x;
  const auto par = [t](auto f) {
    f(t);
    __syncthreads();
  };
  for (int32_t j = (int32_t)blockIdx.x; j < A.n_scalar; j += (int32_t)gridDim.x) {
    for (int32_t i = t; i < A.n_pad; i += T) keys[i] = spicey_tmc_key_of(A, i, j);
    __syncthreads();
    spicey_mc_sort(par, T, keys, A.n_pad);
    const int32_t n_num = spicey_tmc_count_below(keys, A.n_pad, SPICEY_TMC_NAN_KEY);
    const int32_t n_valid = spicey_tmc_count_below(keys, A.n_pad, SPICEY_MC_PAD_KEY);
    if (t < SPICEY_MC_LANES) {
      SpiceyTmcPartial p;
      spicey_tmc_stat_lane(A, j, keys, n_valid, n_num, t, &p);
      // p[l] meets p[l + stride] for l < stride; the lanes above take what no later stride reads
      for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1) spicey_tmc_stat_meet(&p, tmc_shfl_down(p, stride));
      if (t == 0) spicey_tmc_stat_row(A, j, n_valid, n_num, p, stat);
    }
    spicey_tmc_stat_ranks(A, j, keys, n_num, t, T, stat);
    __syncthreads();  // (the next scalar's keys overwrite these)
  }
}

}  // namespace

hipError_t spicey_launch_tmc_draw(int device, const SpiceyMcDrawArgs &A0, const double *tol, const double *icdf, void *d_work, hipStream_t st) {
  hipError_t e;
  const int32_t nE = A0.nR + A0.nC + A0.nL;
  const size_t off_tol = (size_t)spicey_mc_draw_tol_offset(), off_icdf = (size_t)spicey_mc_draw_icdf_offset(nE);
  const size_t n_tab = ((size_t)1 << A0.log2K) + 1;
  // (the record, the tolerances and the table in one copy: the record names their places behind it)
  SpiceyMcDrawArgs A = A0;
  A.tol = (const double *)((const char *)d_work + off_tol);
  A.icdf = (const double *)((const char *)d_work + off_icdf);
  std::vector<char> head(off_icdf + n_tab * sizeof(double), 0);
  memcpy(head.data(), &A, sizeof(A));
  memcpy(head.data() + off_tol, tol, (size_t)nE * sizeof(double));
  memcpy(head.data() + off_icdf, icdf, n_tab * sizeof(double));
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const int64_t total = (int64_t)A.n_inst * (int64_t)nE;
  unsigned grid = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MC_THREADS, &grid)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_tmc_draw_kernel, dim3(grid), dim3(SPICEY_MC_THREADS), 0, st, (const SpiceyMcDrawArgs *)d_work, total);
  return hipGetLastError();
}

hipError_t spicey_launch_tmc_scalars(int device, const SpiceyTmcArgs &A0, const SpiceyMcScalar *scalars, const uint8_t *valid, const double *lo, const double *hi,
                                     const double *probs, double *d_x, void *d_work, hipStream_t st) {
  hipError_t e;
  SpiceyTmcLayout l;
  if (!spicey_tmc_layout(A0.n_inst, A0.n_scalar, A0.n_prob, l)) return hipErrorInvalidValue;
  SpiceyTmcArgs A = A0;
  std::vector<char> head((size_t)l.total_bytes);
  spicey_tmc_head(l, A, scalars, valid, lo, hi, probs, d_x, head.data(), (char *)d_work);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const int64_t total = (int64_t)A.n_inst * (int64_t)A.n_scalar;
  unsigned grid = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MC_THREADS, &grid)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_tmc_scalar_kernel, dim3(grid), dim3(SPICEY_MC_THREADS), 0, st, (const SpiceyTmcArgs *)d_work, total);
  return hipGetLastError();
}

hipError_t spicey_launch_tmc_reduce(int device, const SpiceyTmcArgs &A, const SpiceyMcScalar *scalars, const uint8_t *valid, const double *lo, const double *hi,
                                    const double *probs, double *d_x, double *d_stat, int64_t *d_sample, void *d_work, hipStream_t st) {
  hipError_t e;
  if ((e = spicey_launch_tmc_scalars(device, A, scalars, valid, lo, hi, probs, d_x, d_work, st)) != hipSuccess) return e;
  const SpiceyTmcArgs *d_A = (const SpiceyTmcArgs *)d_work;
  unsigned grid = 0;
  if ((e = spicey_meas_grid2(A.n_inst, SPICEY_MC_THREADS, &grid)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_tmc_sample_kernel, dim3(grid), dim3(SPICEY_MC_THREADS), 0, st, d_A, d_sample);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const size_t lds = (size_t)A.n_pad * sizeof(uint64_t);
  if ((e = spicey_allow_dyn_lds(spicey_tmc_stat_kernel, lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_tmc_stat_kernel, dim3(spicey_meas_grid1(A.n_scalar)), dim3(A.sort_threads), lds, st, d_A, d_stat);
  return hipGetLastError();
}
