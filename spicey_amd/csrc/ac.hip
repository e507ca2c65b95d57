// ac.hip — AC sweep on the GPU: kernels and launchers (the C-ABI spicey_ac_* of include/spicey_hip.h is ac_abi.cpp).
//
// One workgroup per (instance, frequency) pair runs a whole complex MNA solve (ac_exec.h): the pairs are
// independent (simulateAC.ts:80 `for (const f of freqs)`), so the sweep is one launch of n_inst * n_freq workgroups.
// Workspace: nW complex entries = 16 bytes each, in LDS when it fits (<= ~10 000 entries), else one slice of a global
// buffer per workgroup.  The schedule ("program") is the transient one of symbolic.cpp built from the descriptor
// without diodes and switches.
#include <hip/hip_runtime.h>

#include "ac_exec.h"
#include "kernels.h"

namespace {

struct GpuAcExec {
  __device__ __forceinline__ int threads() const { return (int)blockDim.x; }
  __device__ __forceinline__ int atomic_inc(int32_t *p) { return atomicAdd(p, 1); }
  template <class F>
  __device__ __forceinline__ void phase(int, F f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

template <class Regs>
struct GpuAcExecRes {
  Regs rr;
  __device__ __forceinline__ int threads() const { return (int)blockDim.x; }
  template <class R2>
  __device__ __forceinline__ R2 &regs(int) { return rr; }
  template <class F>
  __device__ __forceinline__ void phase(int, F f) {
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));  // (keeps per-thread addresses from being hoisted out of the frequency loop)
    f(tid);
    __syncthreads();
  }
};

// Resident sweep: blockIdx.x = instance * n_chunk + c; the workgroup runs frequencies c, c + n_chunk, ... of its instance
// with the task records and the frequency-independent stamp parts in registers (ac_exec.h).
// INJ: the build with the current injection of SpiceyAcRun::inj_* (both sweep kernels exist twice: the arguments arrive in
// scalar registers, and the build without injection never reads the fields — it is the kernel of every plain run, with the
// registers and the code it had before).
template <int RMAX, int NSE, bool INJ>
__global__ void __launch_bounds__(512) spicey_ac_kernel_res(SpiceyProg P, SpiceyResident Q, SpiceyAcRun R, int n_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int32_t flags[2];
  GpuAcExecRes<AcResRegs<RMAX, NSE>> ex;
  spicey_ac_sweep_resident<RMAX, NSE, INJ>(ex, P, Q, R, (SpiceyCx *)smem, flags, (size_t)(blockIdx.x / (unsigned)n_chunk), (int64_t)(blockIdx.x % (unsigned)n_chunk),
                                      (int64_t)n_chunk);
}

template <bool LDS, bool INJ>
__global__ void __launch_bounds__(1024) spicey_ac_kernel(SpiceyProg P, SpiceyAcRun R) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int32_t flags[2];
  const int64_t slot = R.slot_base + (int64_t)blockIdx.x;
  SpiceyCx *W = LDS ? (SpiceyCx *)smem : (SpiceyCx *)R.gW + (size_t)blockIdx.x * (size_t)P.nW;
  GpuAcExec ex;
  spicey_ac_solve<INJ>(ex, P, R, W, flags, slot);
}

// Dense partial-pivoting fallback (ac_exec.h): blockIdx.x = index into the list of (instance, frequency) slots whose solve
// tripped a pivot guard; A | b and the sparse scratch of each in global memory, reduction scratch in LDS.
__global__ void __launch_bounds__(1024) spicey_ac_dense_kernel(const SpiceyProg *__restrict__ Pp, const SpiceyAcRun *__restrict__ Rp, const int64_t *slots,
                                                                SpiceyCx *Ws_all, SpiceyCx *A_all) {
  // (the two argument structs by pointer: by value their ~110 fields are all live SGPRs and some spill)
  const SpiceyProg &P = *Pp;
  const SpiceyAcRun &R = *Rp;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int32_t flags[2];
  const int T = (int)blockDim.x, n = P.n;
  double *sd = (double *)smem;
  int32_t *si = (int32_t *)(sd + (size_t)T + 2 * (size_t)n + 2);
  GpuAcExec ex;
  spicey_ac_dense_solve(ex, P, R, Ws_all + (size_t)blockIdx.x * (size_t)P.nW, A_all + (size_t)blockIdx.x * (size_t)n * ((size_t)n + 1), sd, si, flags,
                        slots[blockIdx.x]);
}

}  // namespace

hipError_t spicey_launch_ac_resident(const SpiceyProg &P, const SpiceyResident &Q, const SpiceyAcRun &R, int n_chunk, int threads, size_t lds_bytes, hipStream_t st) {
  const bool inj = (R.inj_p | R.inj_n) != 0;
  auto kern = inj ? spicey_ac_kernel_res<SPICEY_AC_RMAX, SPICEY_AC_NSE, true> : spicey_ac_kernel_res<SPICEY_AC_RMAX, SPICEY_AC_NSE, false>;
  if (const hipError_t e = spicey_allow_dyn_lds(kern, lds_bytes); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(R.n_inst * n_chunk)), dim3(threads), lds_bytes, st, P, Q, R, n_chunk);
  return hipGetLastError();
}

hipError_t spicey_launch_ac(const SpiceyProg &P, const SpiceyAcRun &R, int grid, int threads, size_t lds_bytes, hipStream_t st) {
  const bool inj = (R.inj_p | R.inj_n) != 0;
  if (lds_bytes) {
    auto kern = inj ? spicey_ac_kernel<true, true> : spicey_ac_kernel<true, false>;
    if (const hipError_t e = spicey_allow_dyn_lds(kern, lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds_bytes, st, P, R);
  } else {
    auto kern = inj ? spicey_ac_kernel<false, true> : spicey_ac_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), 0, st, P, R);
  }
  return hipGetLastError();
}

hipError_t spicey_launch_ac_dense(const SpiceyProg *P, const SpiceyAcRun *R, int n, const int64_t *d_slots, int count, SpiceyCx *Ws, SpiceyCx *A, hipStream_t st) {
  const int Td = 1024;
  const size_t lds = ((size_t)Td + 2 * (size_t)n + 2) * sizeof(double) + ((size_t)Td + (size_t)n + 4) * sizeof(int32_t);
  if (const hipError_t e = spicey_allow_dyn_lds(spicey_ac_dense_kernel, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_ac_dense_kernel, dim3((unsigned)count), dim3(Td), lds, st, P, R, d_slots, Ws, A);
  return hipGetLastError();
}
