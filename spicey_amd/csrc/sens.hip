// sens.hip — first-order AC sensitivities reduced on the device (spicey_ac_sens_device, spicey_ac_run_sens): kernels and
// launcher.
//
// A reduction pass over the complex buffers [inst][freq][col][2] a plain and an injected sweep wrote; sens_exec.h holds the
// arithmetic, the mapping and the summation order, shared with the CPU harness of tests/sens_host.  Two kernels, no LDS, no
// barrier, no atomics, nothing waits for another workgroup:
//   spectrum  one wave per (instance, frequency): lane l reads the 16 bytes of element l, l + 64, ... of the slot's rows of
//             both sweeps' currents, 8 bytes of the element's value and 8 of its tolerance — neighbouring lanes read
//             neighbouring addresses, a 1 KiB row segment per 16-byte wave instruction — and adds its four sums in ascending e;
//             the 64 partials of each sum meet by s[l] += s[l + stride], stride 32 .. 1, through __shfl_down (ds_bpermute_b32,
//             two per double and stride, as noise.hip: the pass is bound by the one read of the two rows).  Lane 0 writes the
//             slot's row of d_spec; with d_full every lane writes the 16 bytes {m, phi} of its elements, consecutive again.
//   peak      one thread per (instance, element) walks the window re-reading its own column of both sweeps (neighbouring
//             threads read neighbouring elements of one k) and keeps the value of largest magnitude.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit (as noise.hip); f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "measure.h"
#include "sens.h"

namespace {

static_assert(SPICEY_SENS_LANES == 64, "one slot per wave: gfx950 waves have 64 lanes");

__global__ void __launch_bounds__(SPICEY_SENS_THREADS) spicey_sens_spectrum_kernel(const SpiceySensArgs *__restrict__ Ap, double *__restrict__ spec,
                                                                                  double *__restrict__ full) {
  const SpiceySensArgs A = *Ap;
  const int lane = (int)(threadIdx.x & (SPICEY_SENS_LANES - 1));
  // (the wave's number is the same in all its lanes: as a scalar, so is the slot)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SPICEY_SENS_LANES));
  const int per_wg = SPICEY_SENS_THREADS / SPICEY_SENS_LANES;
  const int64_t slots = (int64_t)A.n_inst * A.n_freq;
  for (int64_t slot = (int64_t)blockIdx.x * per_wg + wave; slot < slots; slot += (int64_t)gridDim.x * per_wg) {
    double s[4];
    spicey_sens_lane(A, slot, lane, full, s);
    // s[l] += s[l + stride] for l < stride; the lanes above add what no later stride reads
    for (int stride = SPICEY_SENS_LANES / 2; stride > 0; stride >>= 1) {
      s[0] = s[0] + __shfl_down(s[0], stride);
      s[1] = s[1] + __shfl_down(s[1], stride);
      s[2] = s[2] + __shfl_down(s[2], stride);
      s[3] = s[3] + __shfl_down(s[3], stride);
    }
    if (lane == 0) spicey_sens_spec_row(A, slot, s, spec);
  }
}

__global__ void __launch_bounds__(SPICEY_SENS_THREADS) spicey_sens_peak_kernel(const SpiceySensArgs *__restrict__ Ap, int64_t total_threads,
                                                                              double *__restrict__ peak) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_SENS_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceySensArgs A = *Ap;
  spicey_sens_peak(A, idx, peak);
}

}  // namespace

hipError_t spicey_launch_sens(int device, const SpiceySensArgs &A0, const double *tol, double *d_spec, double *d_peak, double *d_full, void *d_work, hipStream_t st) {
  hipError_t e;
  const int32_t nE = A0.nR + A0.nC + A0.nL;
  const size_t off = (size_t)spicey_sens_tol_offset();
  // (the record and the tolerances in one copy: the record names the tolerances' place behind it)
  SpiceySensArgs A = A0;
  A.tol = (const double *)((const char *)d_work + off);
  std::vector<char> head(off + (size_t)nE * sizeof(double), 0);
  memcpy(head.data(), &A, sizeof(A));
  memcpy(head.data() + off, tol, (size_t)nE * sizeof(double));
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const SpiceySensArgs *d_A = (const SpiceySensArgs *)d_work;
  const int64_t slots = (int64_t)A.n_inst * A.n_freq, per_wg = SPICEY_SENS_THREADS / SPICEY_SENS_LANES;
  hipLaunchKernelGGL(spicey_sens_spectrum_kernel, dim3(spicey_meas_grid1((slots + per_wg - 1) / per_wg)), dim3(SPICEY_SENS_THREADS), 0, st, d_A, d_spec, d_full);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t total = (int64_t)A.n_inst * (int64_t)nE;
  unsigned grid2 = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_SENS_THREADS, &grid2)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_sens_peak_kernel, dim3(grid2), dim3(SPICEY_SENS_THREADS), 0, st, d_A, total, d_peak);
  return hipGetLastError();
}
