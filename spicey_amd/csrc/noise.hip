// noise.hip — thermal noise of an injected AC sweep reduced on the device (spicey_ac_noise_device, spicey_ac_run_noise):
// kernels and launcher.
//
// A reduction pass over the complex buffers [inst][freq][col][2] an injected sweep wrote; noise_exec.h holds the arithmetic,
// the mapping and the summation order, shared with the CPU harness of tests/noise_host.  Two kernels, no LDS, no barrier, no
// atomics, nothing waits for another workgroup:
//   spectrum  one wave per (instance, frequency): lane l reads the 16 bytes of resistor l, l + 64, ... of the slot's row of
//             currents — neighbouring lanes read neighbouring 16 bytes, one 1 KiB row segment per wave instruction — adds
//             kt4 R |i|^2 in ascending r, and the 64 partials meet by s[l] += s[l + stride], stride 32 .. 1.  The moves are
//             __shfl_down (ds_bpermute_b32, two per double and stride): the pass is bound by the one read of the row, six
//             strides of two LDS-crossbar moves are noise beside it, and unlike a DPP row shift the same instruction serves
//             the strides 32 and 16 that leave a row of 16 lanes.  Lane 0 writes the slot's row of d_spec.
//   band      one thread per (instance, row): the resistors' rows walk the window re-reading their own column (neighbouring
//             threads read neighbouring resistors), the two last rows walk d_spec.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit (as ac_measure.hip); f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "measure.h"
#include "noise.h"

namespace {

static_assert(SPICEY_NOISE_LANES == 64, "one slot per wave: gfx950 waves have 64 lanes");

__global__ void __launch_bounds__(SPICEY_NOISE_THREADS) spicey_noise_spectrum_kernel(const SpiceyNoiseArgs *__restrict__ Ap, double *__restrict__ spec) {
  const SpiceyNoiseArgs A = *Ap;
  const int lane = (int)(threadIdx.x & (SPICEY_NOISE_LANES - 1));
  // (the wave's number is the same in all its lanes: as a scalar, so is the slot)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SPICEY_NOISE_LANES));
  const int per_wg = SPICEY_NOISE_THREADS / SPICEY_NOISE_LANES;
  const int64_t slots = (int64_t)A.n_inst * A.n_freq;
  for (int64_t slot = (int64_t)blockIdx.x * per_wg + wave; slot < slots; slot += (int64_t)gridDim.x * per_wg) {
    double s = spicey_noise_lane(A, slot, lane);
    // s[l] += s[l + stride] for l < stride; the lanes above add what no later stride reads
    for (int stride = SPICEY_NOISE_LANES / 2; stride > 0; stride >>= 1) s = s + __shfl_down(s, stride);
    if (lane == 0) spicey_noise_spec_row(A, slot, s, spec);
  }
}

__global__ void __launch_bounds__(SPICEY_NOISE_THREADS) spicey_noise_band_kernel(const SpiceyNoiseArgs *__restrict__ Ap, int64_t total_threads,
                                                                                const double *__restrict__ spec, double *__restrict__ contrib,
                                                                                double *__restrict__ total) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_NOISE_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceyNoiseArgs A = *Ap;
  spicey_noise_band(A, idx, spec, contrib, total);
}

}  // namespace

hipError_t spicey_launch_noise(int device, const SpiceyNoiseArgs &A, double *d_spec, double *d_contrib, double *d_total, void *d_work, hipStream_t st) {
  hipError_t e;
  if ((e = spicey_upload_table_async(device, d_work, &A, sizeof(A), st)) != hipSuccess) return e;
  const SpiceyNoiseArgs *d_A = (const SpiceyNoiseArgs *)d_work;
  const int64_t slots = (int64_t)A.n_inst * A.n_freq, per_wg = SPICEY_NOISE_THREADS / SPICEY_NOISE_LANES;
  hipLaunchKernelGGL(spicey_noise_spectrum_kernel, dim3(spicey_meas_grid1((slots + per_wg - 1) / per_wg)), dim3(SPICEY_NOISE_THREADS), 0, st, d_A, d_spec);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t total = (int64_t)A.n_inst * ((int64_t)A.nR + 2);
  unsigned grid2 = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_NOISE_THREADS, &grid2)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_noise_band_kernel, dim3(grid2), dim3(SPICEY_NOISE_THREADS), 0, st, d_A, total, (const double *)d_spec, d_contrib, d_total);
  return hipGetLastError();
}
