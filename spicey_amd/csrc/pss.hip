// pss.hip — periodic steady state by shooting Newton on the device (spicey_pss_design_device, spicey_pss_update_device,
// spicey_run_pss): kernels and launchers.
//
// pss_exec.h holds the arithmetic, the mapping and the order, shared with the CPU harness of tests/pss_host.  Two kernels, no
// atomics, nothing waits for another workgroup:
//   design   one thread per (instance, state entry): one load, for a perturbed entry a product, a sum and a difference, one or
//            two stores; the thread of entry 0 copies the circuit's switch states into its instance.
//   update   one workgroup of 256 per circuit.  The matrix I - J with the residual as its last column lives in dynamic LDS, row
//            stride nX + 1 doubles — 132 096 bytes at nX = 128, an odd stride at even nX, so a column's rows spread over the
//            banks —; Gaussian elimination with partial pivoting runs in it, the pivot searched by the first wave (two rows per
//            lane at most, met by __shfl_down, stride 32 .. 1), rows in parallel, the column index sequential, barriers between;
//            then the column-oriented back substitution and the move of the base.  One circuit's update is a few hundred
//            barriers on at most 16 512 doubles: latency-bound, and as long as one period of one instance at most.
// Bit identity with the CPU harness needs every product, sum and quotient rounded on its own: no FMA contraction in this
// translation unit; f64 division is the correctly rounded sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "devbuf.h"
#include "measure.h"
#include "pss.h"

namespace {

static_assert(SPICEY_PSS_LANES == 64, "the pivot's wave: gfx950 waves have 64 lanes");
static_assert(2 * SPICEY_PSS_LANES >= SPICEY_PSS_MAX_NX && SPICEY_PSS_THREADS >= SPICEY_PSS_LANES, "one wave searches a column");

__global__ void __launch_bounds__(SPICEY_PSS_THREADS) spicey_pss_design_kernel(const SpiceyPssArgs *__restrict__ Ap, int64_t total_threads) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_PSS_THREADS + threadIdx.x;
  if (idx >= total_threads) return;
  const SpiceyPssArgs A = *Ap;
  spicey_pss_design(A, idx);
}

// The workgroup as spicey_pss_update sees it.
struct PssWorkgroup {
  int32_t T;
  template <class F>
  __device__ __forceinline__ void par(F f) {
    f((int32_t)threadIdx.x);
    __syncthreads();
  }
  __device__ __forceinline__ void pivot(const double *M, int32_t nX, int32_t k, SpiceyPssShared *sh) {
    if (threadIdx.x < SPICEY_PSS_LANES) {  // (the whole first wave: no lane is missing from the shuffles)
      SpiceyPssPiv p = spicey_pss_piv_lane(M, nX, k, (int32_t)threadIdx.x);
      for (int stride = SPICEY_PSS_LANES / 2; stride > 0; stride >>= 1) {
        SpiceyPssPiv q;
        q.v = __shfl_down(p.v, stride);
        q.i = __shfl_down(p.i, stride);
        spicey_pss_piv_meet(&p, q);
      }
      if (threadIdx.x == 0) spicey_pss_piv_done(sh, k, p);
    }
    __syncthreads();
  }
};

__global__ void __launch_bounds__(SPICEY_PSS_THREADS) spicey_pss_update_kernel(const SpiceyPssArgs *__restrict__ Ap) {
  extern __shared__ double pss_matrix[];
  __shared__ SpiceyPssShared sh;
  const SpiceyPssArgs A = *Ap;
  const int32_t c = (int32_t)blockIdx.x;
  if (c >= A.n_ckt) return;
  PssWorkgroup wg{SPICEY_PSS_THREADS};
  spicey_pss_update(A, c, pss_matrix, &sh, wg);
}

hipError_t upload_head(int device, const SpiceyPssArgs &A0, const int32_t *ist, void *d_work, hipStream_t st) {
  SpiceyPssLayout l;
  if (!spicey_pss_layout(A0.n_ckt, spicey_pss_nx(A0), A0.method, l)) return hipErrorInvalidValue;
  SpiceyPssArgs A = A0;
  std::vector<char> head((size_t)l.total_bytes);
  spicey_pss_head(l, A, ist, head.data(), (char *)d_work);
  // (without statuses the record alone goes up)
  return spicey_upload_table_async(device, d_work, head.data(), ist ? head.size() : sizeof(SpiceyPssArgs), st);
}

}  // namespace

hipError_t spicey_launch_pss_design(int device, const SpiceyPssArgs &A, void *d_work, hipStream_t st) {
  hipError_t e;
  if ((e = upload_head(device, A, nullptr, d_work, st)) != hipSuccess) return e;
  const int32_t nX = spicey_pss_nx(A);
  const int64_t total = (int64_t)A.n_ckt * spicey_pss_w(A) * nX;
  unsigned grid = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_PSS_THREADS, &grid)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_pss_design_kernel, dim3(grid), dim3(SPICEY_PSS_THREADS), 0, st, (const SpiceyPssArgs *)d_work, total);
  return hipGetLastError();
}

hipError_t spicey_launch_pss_update(int device, const SpiceyPssArgs &A, const int32_t *ist, void *d_work, hipStream_t st) {
  hipError_t e;
  if ((e = upload_head(device, A, ist, d_work, st)) != hipSuccess) return e;
  const size_t lds = spicey_pss_lds_bytes(A.method, spicey_pss_nx(A));
  if ((e = spicey_allow_dyn_lds(spicey_pss_update_kernel, lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_pss_update_kernel, dim3((unsigned)A.n_ckt), dim3(SPICEY_PSS_THREADS), lds, st, (const SpiceyPssArgs *)d_work);
  return hipGetLastError();
}
