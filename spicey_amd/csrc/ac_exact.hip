// ac_exact.hip — the reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3): kernel and launcher
// (the handle is ac_abi.cpp's).
//
// One workgroup per (instance, frequency) slot runs ac_exact_exec.h, the reference's own algorithm (fresh dense complex
// stamp, solveComplex with partial pivoting on V8's Math.hypot and its |f| < EPS skip, back substitution in its order).
// Bit identity with the reference needs every product and sum rounded on its own: this translation unit is compiled
// without FMA contraction (the pragma below; hipcc contracts by default, and the other kernels keep doing so).  f64
// division is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence and sqrt the correctly rounded
// expansion of llvm.sqrt.f64.  Workspace: A | b, x, the quantities, multipliers, permutation and active rows in LDS when
// they fit (n up to ~97), else the slot's slab of a global buffer.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>

#include "ac_exact_exec.h"
#include "kernels.h"

namespace {

// (the pivot search of GpuExactExec in exact.hip, on the same total order)
struct GpuAcExactExec {
  double *red_v;  // [16] per-wave maxima of the pivot search
  int32_t *red_i;
  __device__ __forceinline__ int threads() const { return (int)blockDim.x; }
  __device__ __forceinline__ int atomic_add(int32_t *p, int v) { return atomicAdd(p, v); }
  template <class F>
  __device__ __forceinline__ void phase(int, F f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
  // first strict maximum: each thread scans its rows in ascending order, then (value, index) pairs are combined by "larger
  // value, or equal value and lower index" — a total order, so the result does not depend on how the pairs meet.  One
  // wave: cross-lane moves only, no barrier; more: one LDS slot per wave and one barrier.  (The next writer of red_v is the
  // next pivot search, behind at least one phase barrier.)
  template <class G>
  __device__ __forceinline__ void argmax(int count, G get, double &bv, int &bi) {
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    double v = -1.0;
    int i = INT_MAX;
    for (int j = tid; j < count; j += T) {
      const double g = get(j);
      if (g > v) { v = g; i = j; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double v2 = __shfl_xor(v, off);
      const int i2 = __shfl_xor(i, off);
      if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
    }
    if (T > 64) {
      if ((tid & 63) == 0) { red_v[tid >> 6] = v; red_i[tid >> 6] = i; }
      __syncthreads();
      v = red_v[0];
      i = red_i[0];
      for (int w = 1; w < (T >> 6); w++) {
        const double v2 = red_v[w];
        const int i2 = red_i[w];
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
      }
    }
    bv = v;
    bi = i;
  }
};

// blockIdx.x = slot - slot_base (slots instance-major).  The argument structs by pointer (by value their fields would all
// be live SGPRs).
__global__ void __launch_bounds__(1024) spicey_ac_exact_kernel(const SpiceyAcExactProg *__restrict__ Pp, const SpiceyAcExactRun *__restrict__ Rp,
                                                                int64_t slot_base, int use_lds) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double red_v[16];
  __shared__ int32_t red_i[16];
  __shared__ int32_t scal[4];
  const SpiceyAcExactProg &P = *Pp;
  const SpiceyAcExactRun &R = *Rp;
  SpiceyCx *ws = use_lds ? (SpiceyCx *)smem : R.gW + (size_t)blockIdx.x * (size_t)P.ws_cx;
  GpuAcExactExec ex{red_v, red_i};
  spicey_ac_exact_solve(ex, P, R, ws, scal, slot_base + (int64_t)blockIdx.x);
}

}  // namespace

hipError_t spicey_launch_ac_exact(const SpiceyAcExactProg *P, const SpiceyAcExactRun *R, int64_t slot_base, int grid, int threads, size_t lds,
                                  hipStream_t st) {
  if (const hipError_t e = spicey_allow_dyn_lds(spicey_ac_exact_kernel, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_ac_exact_kernel, dim3(grid), dim3(threads), lds, st, P, R, slot_base, lds > 0 ? 1 : 0);
  return hipGetLastError();
}
