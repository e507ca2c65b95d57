// ac_exact.hip — the reference-order AC engine (spicey_ac_create with SpiceyOptions.interpreter = 3): kernel, launcher and
// the host side of an exact AC handle (spicey_ac_* of ac.hip hand such a handle to the functions at the end).
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

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "ac_exact_exec.h"
#include "ac_sweep.h"
#include "devbuf.h"
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
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(spicey_ac_exact_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(spicey_ac_exact_kernel, dim3(grid), dim3(threads), lds, st, P, R, slot_base, lds > 0 ? 1 : 0);
  return hipGetLastError();
}

// ---- host side of an exact AC handle ---------------------------------------------------------------------------------

struct SpiceyAcExact {
  AcExactPlan plan;
  HostAcExactProg xp;
  int device = 0, n_inst = 0;
  int64_t last_slots = 0;  // (instance, frequency) slots of the last run
  DevBuf<uint8_t> d_blob;
  DevBuf<SpiceyAcExactProg> d_P;
  DevBuf<double> d_R, d_C, d_L;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;
};

void spicey_ac_exact_destroy(SpiceyAcExact *x) {
  if (!x) return;
  if (x->ev0) (void)hipEventDestroy(x->ev0);
  if (x->ev1) (void)hipEventDestroy(x->ev1);
  if (x->stream) (void)hipStreamDestroy(x->stream);
  delete x;  // (and with it every device buffer)
}

int32_t spicey_ac_exact_create(const SpiceyDesc *desc, const SpiceyOptions &opt, SpiceyAcExact **out, std::string &err) {
  *out = nullptr;
  SpiceyAcExact *x = new SpiceyAcExact();
  auto fail = [&](int32_t code, const std::string &msg) {
    err = msg;
    spicey_ac_exact_destroy(x);
    return code;
  };
  int32_t rc = spicey_ac_exact_plan(desc, opt, x->plan, err);
  if (rc != SPICEY_OK) return fail(rc, err);
  x->n_inst = desc->n_inst;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SPICEY_ERR_NO_DEVICE, "no HIP device: libspicey_hip has no CPU path");
  x->device = opt.device;
  if (x->device < 0 || x->device >= ndev) return fail(SPICEY_ERR_BAD_DESC, "device ordinal out of range");
  if (hipSetDevice(x->device) != hipSuccess) return fail(SPICEY_ERR_HIP, "hipSetDevice failed");
  SpiceyDesc d = *desc;  // (R, C, L and V only)
  d.nS = 0;
  d.nD = 0;
  spicey_build_ac_exact(d, x->plan.ws, x->xp);
  if (dev_upload(x->d_blob, x->xp.blob.size() * sizeof(uint32_t), reinterpret_cast<const uint8_t *>(x->xp.blob.data())) != hipSuccess)
    return fail(SPICEY_ERR_HIP, "upload of the stamp lists failed");
  const SpiceyAcExactProg P = x->xp.bind(x->d_blob);
  if (dev_upload(x->d_P, 1, &P) != hipSuccess) return fail(SPICEY_ERR_HIP, "upload of the program header failed");
  const size_t ni = (size_t)x->n_inst;
  std::vector<double> rinv(ni * (size_t)d.nR);
  for (size_t i = 0; i < rinv.size(); i++) rinv[i] = 1.0 / desc->R_val[i];  // (1 / R in simulateAC.ts:39-41, the same quotient)
  if (dev_upload(x->d_R, rinv.size(), rinv.data()) != hipSuccess || dev_upload(x->d_C, ni * d.nC, desc->C_val) != hipSuccess ||
      dev_upload(x->d_L, ni * d.nL, desc->L_val) != hipSuccess)
    return fail(SPICEY_ERR_HIP, "upload of the element values failed");
  if (hipStreamCreate(&x->stream) != hipSuccess || hipEventCreate(&x->ev0) != hipSuccess || hipEventCreate(&x->ev1) != hipSuccess)
    return fail(SPICEY_ERR_HIP, "stream/event creation failed");
  *out = x;
  return SPICEY_OK;
}

void spicey_ac_exact_info(const SpiceyAcExact *x, SpiceyInfo *info) {
  memset(info, 0, sizeof(*info));
  const SpiceyAcExactProg &H = x->xp.hdr;
  info->n_var = H.n;
  info->threads = x->plan.T;
  info->inst_per_wg = 1;
  info->lds_bytes = x->plan.lds ? (int32_t)x->plan.lds_bytes : 0;
  info->n_cur = H.nCur;
  info->n_out = H.nOut;
  info->n_workgroups = (int32_t)x->last_slots;
  info->interpreter = 3;
  info->wgs_per_inst = 1;
  info->program_bytes = (int64_t)(x->xp.blob.size() * sizeof(uint32_t));
}

const char *spicey_ac_exact_error(const SpiceyAcExact *x) { return x->err.c_str(); }

#define XCHK(call) HIPCHK(x, call)

hipStream_t spicey_ac_exact_stream(const SpiceyAcExact *x) { return x->stream; }
void spicey_ac_exact_dims(const SpiceyAcExact *x, int32_t *n_inst, int32_t *n_out, int32_t *n_cur, int32_t *n_v) {
  *n_inst = x->n_inst;
  *n_out = x->xp.hdr.nOut;
  *n_cur = x->xp.hdr.nCur;
  *n_v = x->xp.hdr.nV;
}

// The sweep into device buffers: every slot solved, o.status on the host, the stream idle.  The caller copies out or reduces.
int32_t spicey_ac_exact_sweep(SpiceyAcExact *x, int64_t n_freq, const double *freqs, const double *vph, bool want_i, SpiceyAcSweep &o, double *ms) {
  const SpiceyAcExactProg &H = x->xp.hdr;
  const int64_t slots = (int64_t)x->n_inst * n_freq;
  if (slots > 0x7fffffffll) { x->err = "n_inst * n_freq exceeds the grid limit"; return SPICEY_ERR_BAD_DESC; }
  XCHK(hipSetDevice(x->device));
  const int64_t chunk = spicey_ac_exact_chunk(x->plan, slots);
  o.status.assign((size_t)slots, 0);
  {
    DevBuf<double> d_f, d_ph;
    DevBuf<SpiceyCx> d_gW;
    DevBuf<int32_t> d_status;
    DevBuf<SpiceyAcExactRun> d_run;
    XCHK(d_f.alloc((size_t)n_freq));
    XCHK(d_ph.alloc(std::max<size_t>(1, (size_t)x->n_inst * H.nV * 2)));
    XCHK(o.d_ov.alloc(std::max<size_t>(1, (size_t)slots * H.nOut * 2)));
    if (want_i) XCHK(o.d_oi.alloc(std::max<size_t>(1, (size_t)slots * H.nCur * 2)));
    XCHK(d_status.alloc((size_t)slots));
    if (!x->plan.lds && d_gW.alloc((size_t)chunk * (size_t)H.ws_cx) != hipSuccess) {
      x->err = "allocation of the global slab failed (" + std::to_string((size_t)chunk * (size_t)H.ws_cx * 16) + " bytes)";
      return SPICEY_ERR_HIP;
    }
    XCHK(hipMemcpyAsync(d_f, freqs, (size_t)n_freq * sizeof(double), hipMemcpyHostToDevice, x->stream));
    if (H.nV > 0) XCHK(hipMemcpyAsync(d_ph, vph, (size_t)x->n_inst * H.nV * 2 * sizeof(double), hipMemcpyHostToDevice, x->stream));
    SpiceyAcExactRun R{};
    R.R_inv = x->d_R; R.C_val = x->d_C; R.L_val = x->d_L;
    R.freqs = d_f; R.vph = d_ph; R.out_v = o.d_ov; R.out_i = o.d_oi; R.gW = d_gW; R.status = d_status; R.skipped = nullptr;
    R.n_freq = n_freq; R.n_inst = x->n_inst;
    XCHK(d_run.alloc(1));
    XCHK(hipMemcpyAsync(d_run, &R, sizeof(R), hipMemcpyHostToDevice, x->stream));
    XCHK(hipEventRecord(x->ev0, x->stream));
    for (int64_t base = 0; base < slots; base += chunk)
      XCHK(spicey_launch_ac_exact(x->d_P, d_run, base, (int)std::min(chunk, slots - base), x->plan.T, x->plan.lds_bytes, x->stream));
    XCHK(hipEventRecord(x->ev1, x->stream));
    XCHK(hipMemcpyAsync(o.status.data(), d_status, (size_t)slots * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
    XCHK(hipStreamSynchronize(x->stream));
    float f = 0.f;
    if (hipEventElapsedTime(&f, x->ev0, x->ev1) == hipSuccess) *ms = f;
  }
  x->last_slots = slots;
  return SPICEY_OK;
}
