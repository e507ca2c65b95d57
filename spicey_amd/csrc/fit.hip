// fit.hip — sizing elements to measured goals on the device (spicey_fit_design_device, spicey_fit_update_device,
// spicey_run_fit): kernels and launchers.
//
// fit_exec.h holds the arithmetic, the mapping and the order, shared with the CPU harness of tests/fit_host.  Two kernels, no
// atomics, nothing waits for another workgroup:
//   design   one thread per (instance, element): a look-up of the element among the active ones, one or two loads, one or two
//            products, one store.
//   update   one workgroup of 256 per circuit.  Thread 0 sums the residuals; on an accepted point the normal equations J^T J and
//            -(J^T r) are formed one entry per thread, each looping over the scalars with the rows of x read from global memory,
//            and kept in the workspace.  The damped matrix with its right-hand side lives in dynamic LDS, row stride nA + 1
//            doubles — 132 096 bytes at nA = 128, an odd stride at even nA, so a column's rows spread over the banks —; Gaussian
//            elimination with partial pivoting runs in it, the pivot searched by the first wave (two rows per lane at most, met
//            by __shfl_down, stride 32 .. 1), barriers between the columns; then the column-oriented back substitution and the
//            step.  A few hundred barriers on at most 16 512 doubles: latency-bound, as the update of pss.hip.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit; f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "devbuf.h"
#include "measure.h"
#include "fit.h"

namespace {

static_assert(SPICEY_FIT_LANES == 64, "the pivot's wave: gfx950 waves have 64 lanes");
static_assert(2 * SPICEY_FIT_LANES >= SPICEY_FIT_MAX_NA && SPICEY_FIT_THREADS >= SPICEY_FIT_LANES, "one wave searches a column");

__global__ void __launch_bounds__(SPICEY_FIT_THREADS) spicey_fit_design_kernel(const SpiceyFitArgs *__restrict__ Ap, int64_t total_threads) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_FIT_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceyFitArgs A = *Ap;
  spicey_fit_design(A, idx);
}

// The workgroup as spicey_fit_update sees it.
struct FitWorkgroup {
  int32_t T;
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int32_t)threadIdx.x);
    __syncthreads();
  }
  __device__ __forceinline__ void pivot(const SpiceyFitArgs &A, const double *M, int32_t k, SpiceyFitShared *sh) {
    if (threadIdx.x < SPICEY_FIT_LANES) {  // (the whole first wave: no lane is missing from the shuffles)
      SpiceyPssPiv p = spicey_pss_piv_lane(M, A.nA, k, (int32_t)threadIdx.x);
      for (int stride = SPICEY_FIT_LANES / 2; stride > 0; stride >>= 1) {
        SpiceyPssPiv q;
        q.v = __shfl_down(p.v, stride);
        q.i = __shfl_down(p.i, stride);
        spicey_pss_piv_meet(&p, q);
      }
      if (threadIdx.x == 0) spicey_fit_piv_done(A, sh, k, p);
    }
    __syncthreads();
  }
};

__global__ void __launch_bounds__(SPICEY_FIT_THREADS) spicey_fit_update_kernel(const SpiceyFitArgs *__restrict__ Ap) {
  extern __shared__ double fit_matrix[];
  __shared__ SpiceyFitShared sh;
  const SpiceyFitArgs A = *Ap;
  const int32_t c = (int32_t)blockIdx.x;
  if (c >= A.n_ckt) return;
  FitWorkgroup wg{SPICEY_FIT_THREADS};
  spicey_fit_update(A, c, fit_matrix, &sh, wg);
}

}  // namespace

hipError_t spicey_launch_fit_design(int device, const SpiceyFitArgs &A0, const int32_t *act, const double *step, void *d_work, hipStream_t st) {
  hipError_t e;
  SpiceyFitLayout l;
  if (!spicey_fit_layout(A0.n_ckt, A0.nA, 1, l)) return hipErrorInvalidValue;
  SpiceyFitArgs A = A0;
  std::vector<char> head((size_t)l.off_rec);
  spicey_fit_design_head(l, A, act, step, head.data(), (char *)d_work);
  if ((e = spicey_upload_table_async(device, d_work, head.data(), head.size(), st)) != hipSuccess) return e;
  const int64_t total = l.n_inst * ((int64_t)A.nR + A.nC + A.nL);
  unsigned grid = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_FIT_THREADS, &grid)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_fit_design_kernel, dim3(grid), dim3(SPICEY_FIT_THREADS), 0, st, (const SpiceyFitArgs *)d_work, total);
  return hipGetLastError();
}

hipError_t spicey_launch_fit_update(int device, const SpiceyFitArgs &A0, const double *step, const double *g_lo, const double *g_hi, const SpiceyFitGoal *goals,
                                    const uint8_t *valid, void *d_work, hipStream_t st, bool staged) {
  hipError_t e;
  SpiceyFitLayout l;
  if (!spicey_fit_layout(A0.n_ckt, A0.nA, A0.n_scalar, l)) return hipErrorInvalidValue;
  SpiceyFitArgs A = A0;
  if (staged) {  // (the arrays of the head are where an earlier launch put them: the record, and the validity where there is one)
    spicey_fit_update_pointers(l, A, valid != nullptr, (char *)d_work);
    if ((e = spicey_upload_table_async(device, (char *)d_work + l.off_rec, &A, sizeof(A), st)) != hipSuccess) return e;
    if (valid && (e = spicey_upload_table_async(device, (char *)d_work + l.off_valid, valid, (size_t)l.n_inst, st)) != hipSuccess) return e;
  } else {
    std::vector<char> head((size_t)(l.off_state - l.off_rec));
    spicey_fit_update_head(l, A, step, g_lo, g_hi, goals, valid, head.data(), (char *)d_work);
    // (without a validity array the head ends before its place)
    if ((e = spicey_upload_table_async(device, (char *)d_work + l.off_rec, head.data(), (size_t)((valid ? l.off_state : l.off_valid) - l.off_rec), st)) != hipSuccess) return e;
  }
  const size_t lds = spicey_fit_lds_bytes(A.nA);
  if ((e = spicey_allow_dyn_lds(spicey_fit_update_kernel, lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_fit_update_kernel, dim3((unsigned)A.n_ckt), dim3(SPICEY_FIT_THREADS), lds, st, (const SpiceyFitArgs *)((const char *)d_work + l.off_rec));
  return hipGetLastError();
}
