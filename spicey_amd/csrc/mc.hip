// mc.hip — Monte Carlo tolerance analysis of the AC sweep on the device (spicey_ac_mc_draw_device, spicey_ac_mc_reduce_device,
// spicey_ac_run_mc): kernels and launchers.
//
// mc_exec.h holds the arithmetic, the mapping and the summation order, shared with the CPU harness of tests/mc_host.  Three
// kernels, no atomics, nothing waits for another workgroup:
//   draw        one thread per (sample, element): ten Philox rounds in 32-bit integer multiplies, one table interpolation, one
//               product (and for a resistor one quotient); neighbouring threads write neighbouring elements of one sample.
//   sample      one wave per sample s < n_pad, lanes striding the frequencies: |H|^2 of the sample's slots as sortable keys into
//               column s of qT [n_freq][n_pad] — the transposition that lets a frequency's workgroup read its row consecutively —
//               and the sample's violations of the mask, which meet across the lanes as integers (__shfl_down).
//   frequency   one workgroup per frequency: the row's n_pad keys into dynamic LDS (8 n_pad bytes, 128 KiB at 16384 samples: one
//               workgroup per CU there), a bitonic network on them as unsigned integers — every stage's n_pad / 2 pairs spread
//               over the threads, a barrier between stages — then wave 0 sums the first n_valid values and their squares in the
//               fixed lane order and every thread writes its share of the order statistics.  Every stage goes through LDS; a
//               cross-lane form of the stages whose partner lies within a wave is not tried here.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit (as sens.hip); f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "devbuf.h"
#include "mc.h"
#include "measure.h"

namespace {

static_assert(SPICEY_MC_LANES == 64, "one sample per wave: gfx950 waves have 64 lanes");

__global__ void __launch_bounds__(SPICEY_MC_THREADS) spicey_mc_draw_kernel(const SpiceyMcDrawArgs *__restrict__ Ap, int64_t total_threads) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MC_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceyMcDrawArgs A = *Ap;
  spicey_mc_draw(A, idx);
}

__global__ void __launch_bounds__(SPICEY_MC_THREADS) spicey_mc_sample_kernel(const SpiceyMcReduceArgs *__restrict__ Ap, int64_t *__restrict__ sample) {
  const SpiceyMcReduceArgs A = *Ap;
  const int lane = (int)(threadIdx.x & (SPICEY_MC_LANES - 1));
  // (the wave's number is the same in all its lanes: as a scalar, so is the sample)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SPICEY_MC_LANES));
  const int per_wg = SPICEY_MC_THREADS / SPICEY_MC_LANES;
  for (int64_t s = (int64_t)blockIdx.x * per_wg + wave; s < A.n_pad; s += (int64_t)gridDim.x * per_wg) {
    int64_t count, first;
    spicey_mc_sample_lane(A, s, lane, &count, &first);
    for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1) {
      const int64_t c2 = __shfl_down((long long)count, stride), f2 = __shfl_down((long long)first, stride);
      spicey_mc_sample_meet(&count, &first, c2, f2);
    }
    if (lane == 0) spicey_mc_sample_row(A, s, count, first, sample);
  }
}

__global__ void __launch_bounds__(SPICEY_MC_SORT_MAX) spicey_mc_freq_kernel(const SpiceyMcReduceArgs *__restrict__ Ap, double *__restrict__ freq) {
  extern __shared__ uint64_t keys[];
  const SpiceyMcReduceArgs A = *Ap;
  const int32_t t = (int32_t)threadIdx.x, T = (int32_t)blockDim.x;
  const auto par = [t](auto f) {
    f(t);
    __syncthreads();
  };
  for (int64_t k = blockIdx.x; k < A.n_freq; k += gridDim.x) {
    const uint64_t *row = A.qT + k * A.n_pad;
    for (int32_t i = t; i < A.n_pad; i += T) keys[i] = row[i];
    __syncthreads();
    spicey_mc_sort(par, T, keys, A.n_pad);
    if (t < SPICEY_MC_LANES) {
      double s[2];
      int64_t viol;
      spicey_mc_freq_lane(A, k, keys, t, s, &viol);
      // s[l] += s[l + stride] for l < stride; the lanes above add what no later stride reads
      for (int stride = SPICEY_MC_LANES / 2; stride > 0; stride >>= 1) {
        s[0] = s[0] + __shfl_down(s[0], stride);
        s[1] = s[1] + __shfl_down(s[1], stride);
        viol += __shfl_down((long long)viol, stride);
      }
      if (t == 0) spicey_mc_freq_row(A, k, s, viol, freq);
    }
    spicey_mc_freq_ranks(A, k, keys, t, T, freq);
    __syncthreads();  // (the next frequency's keys overwrite these)
  }
}

}  // namespace

hipError_t spicey_launch_mc_draw(int device, const SpiceyMcDrawArgs &A0, const double *tol, const double *icdf, void *d_work, hipStream_t st) {
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
  hipLaunchKernelGGL(spicey_mc_draw_kernel, dim3(grid), dim3(SPICEY_MC_THREADS), 0, st, (const SpiceyMcDrawArgs *)d_work, total);
  return hipGetLastError();
}

hipError_t spicey_launch_mc_reduce(int device, const SpiceyMcReduceArgs &A0, const uint8_t *valid, const double *lo, const double *hi, const int64_t *ranks,
                                   int64_t *d_sample, double *d_freq, void *d_work, hipStream_t st) {
  hipError_t e;
  SpiceyMcLayout l;
  if (!spicey_mc_layout(A0.n_inst, A0.n_freq, A0.n_rank, l)) return hipErrorInvalidValue;
  SpiceyMcReduceArgs A = A0;
  std::vector<char> head((size_t)l.head_bytes);
  spicey_mc_reduce_head(l, A, valid, lo, hi, ranks, head.data(), (char *)d_work);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const SpiceyMcReduceArgs *d_A = (const SpiceyMcReduceArgs *)d_work;
  const int64_t per_wg = SPICEY_MC_THREADS / SPICEY_MC_LANES;
  hipLaunchKernelGGL(spicey_mc_sample_kernel, dim3(spicey_meas_grid1((A.n_pad + per_wg - 1) / per_wg)), dim3(SPICEY_MC_THREADS), 0, st, d_A, d_sample);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const size_t lds = (size_t)A.n_pad * sizeof(uint64_t);
  if ((e = spicey_allow_dyn_lds(spicey_mc_freq_kernel, lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_mc_freq_kernel, dim3(spicey_meas_grid1(A.n_freq)), dim3(A.sort_threads), lds, st, d_A, d_freq);
  return hipGetLastError();
}
