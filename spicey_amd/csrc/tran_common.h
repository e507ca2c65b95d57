// tran_common.h — what every executor header shares (tran_exec.h is the map): SPICEY_HD, the device / host macro
// pairs, the phase tags, the workgroup context, and the element models.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "program.h"

#if defined(__HIPCC__)
#define SPICEY_HD __host__ __device__ __forceinline__
#else
#define SPICEY_HD inline
#endif
#ifndef SPICEY_EXP
#define SPICEY_EXP 0  // timing experiments only (tools/exp_build.sh): bit0 no result stores, bit1 no diode section, bit2 no capacitor section, bit3 no parameter loads, bit4 no voltage / resistor section, bit5 no remainder loops
#endif
#ifndef SPICEY_MARK_TID
#define SPICEY_MARK_TID 0
#endif
#if (SPICEY_EXP & 64) && defined(__HIP_DEVICE_COMPILE__)
#define SPICEY_MARK(c, n) do { if ((c).zprof && threadIdx.x == (SPICEY_MARK_TID)) { unsigned long long t_ = clock64(); if ((n) < 15) (c).zprof[n] += t_ - (c).zprof[15]; (c).zprof[15] = t_; } } while (0)
#else
#define SPICEY_MARK(c, n) do { } while (0)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SPICEY_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)  // value is wave-uniform by construction
// Keeps a register-resident packed word packed: without this hipcc hoists the field decode (8+ VGPRs and
// a mask pair per record) out of the time loop and spills.
#define SPICEY_OPAQUE(x) asm volatile("" : "+v"(x))
// Same for wave-uniform values (instance index): per-instance base pointers derived from it are then formed
// inside the phase that needs them instead of living in (spilled) SGPRs across the whole time loop.
#define SPICEY_OPAQUE_S(x) asm volatile("" : "+s"(x))
// wave vote: true if the condition holds in any active lane (a scalar branch: whole waves skip work nobody needs)
#define SPICEY_WAVE_ANY(c) (__builtin_amdgcn_ballot_w64(c) != 0ull)
// result streams are written once and never read by the kernel: non-temporal stores keep them from evicting the
// L2-resident program / parameter lines
#if SPICEY_EXP & 1
#define SPICEY_STREAM_STORE(ptr, val) do { if ((val) == 1.2345e-300) __builtin_nontemporal_store((val), (ptr)); } while (0)
#else
#define SPICEY_STREAM_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
#endif
// diagnostics (SpiceyRun::skip_risk / lin_err): 64-bit integer atomics on global memory; the maximum over a wave by
// cross-lane shuffles (every lane of the wave must arrive: call it outside divergent branches); one lane per wave reports
#define SPICEY_ATOMIC_ADD_U64(p, v) atomicAdd((unsigned long long *)(p), (unsigned long long)(v))
#define SPICEY_ATOMIC_MAX_U64(p, v) atomicMax((unsigned long long *)(p), (unsigned long long)(v))
static __device__ __forceinline__ double spicey_wave_max(double x) {
  for (int off = 32; off > 0; off >>= 1) {
    const double y = __shfl_xor(x, off);
    x = (y > x) ? y : x;
  }
  return x;
}
#define SPICEY_WAVE_MAX(x) spicey_wave_max(x)
#define SPICEY_WAVE_LEADER(tid) (((tid) & 63) == 0)
// cross-lane moves that do not go through the LDS crossbar (used on dependent chains of the dense fronts):
// the value of ONE lane to all (wave-uniform: two v_readlane into scalars) ...
static __device__ __forceinline__ double spicey_readlane_f64(double v, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  asm volatile("" : "+v"(lo), "+v"(hi));  // back into vector registers at once: the kernels that use this have no scalar registers to spare
  return __hiloint2double(hi, lo);
}
// ... and the value of lane q of every quad (4 consecutive lanes) to the quad (DPP quad_perm: a VALU move)
template <int Q>
static __device__ __forceinline__ double spicey_quad_bcast_q(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), Q * 0x55, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), Q * 0x55, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
static __device__ __forceinline__ double spicey_quad_bcast_f64(double v, int q) {
  switch (q & 3) {
    case 0: return spicey_quad_bcast_q<0>(v);
    case 1: return spicey_quad_bcast_q<1>(v);
    case 2: return spicey_quad_bcast_q<2>(v);
    default: return spicey_quad_bcast_q<3>(v);
  }
}
#define SPICEY_NOUNROLL _Pragma("unroll 1")  // thread-strided loops run 1-2 trips: unrolling only costs VGPRs
#define SPICEY_UNROLL _Pragma("unroll")      // small fixed-trip loops over a register array: without it the array is indexed through s_set_gpr_idx
#define SPICEY_SCHED_FENCE __builtin_amdgcn_sched_barrier(0)  // keep the K instances' code from being interleaved
#else
#define SPICEY_NOUNROLL
#define SPICEY_UNROLL
#define SPICEY_SCHED_FENCE
#define SPICEY_UNIFORM(x) (x)
#define SPICEY_OPAQUE(x) (void)(x)
#define SPICEY_OPAQUE_S(x) (void)(x)
#define SPICEY_WAVE_ANY(c) true
#define SPICEY_STREAM_STORE(ptr, val) (*(ptr) = (val))
#define SPICEY_ATOMIC_ADD_U64(p, v) (*(p) += (unsigned long long)(v))
#define SPICEY_ATOMIC_MAX_U64(p, v) do { if ((unsigned long long)(v) > *(p)) *(p) = (unsigned long long)(v); } while (0)
#define SPICEY_WAVE_MAX(x) (x)  // (the emulator runs one thread at a time: every thread reports for itself)
#define SPICEY_WAVE_LEADER(tid) true
#endif

// phase tags (profiling slots, SpiceyRun::prof)
#define SPICEY_PH_PRO 0
#define SPICEY_PH_B 1
#define SPICEY_PH_S 2
#define SPICEY_PH_A 3
#define SPICEY_PH_Z 4
#define SPICEY_PH_Z2 3  // the second phase of a fused Z (tran_v2_run.h: SF) — A's slot: such a run has no switch and never re-iterates
#define SPICEY_PH_U0 8
#define SPICEY_PH_K0 40

template <int K>
struct WgCtx {
  double *W;     // [nW][K]   L+U entries, then rhs / x'
  double *G;     // hybrid workspace (SpiceyProg::hybrid): leaf-owned entries in global memory, [nLU][K] by entry id; else null
  double *u;     // [nU][K]   vPrev | iPrev | V(t) | diode ieq
  double *gd;    // [nGdyn][K] switch conductances | diode gd
  int32_t *ison; // [nS][K]
  int32_t *flags;  // [0] switched, [1] singular code, [2] singular inst
  uint32_t *tail;  // [tail_n][64][4] task records of the tail phases (v2), or null
#if SPICEY_EXP & 64
  unsigned long long *zprof;  // experiment builds: 16 profiling slots for marks inside B / Z ([15] = last timestamp)
#endif
  int32_t inst[K];
  int32_t valid[K];
};

// ---- operand handles (operand-address builds, tran_v2_run.h: OA) ------------------------------------------------------------
// "The double whose index from the start of the workspace is the 16-bit half H of word w."  Through `W[field]` the GPU
// forms its LDS address with two vector instructions — extract the half, then (index << 3) + base, a three-operand add
// even where the base is the constant 0 — in front of every ds_read_b64 of the interpreter.  An OA build states that
// c.W IS LDS address 0 (K = 1, LDS workspace, the dynamic array is the kernel's only LDS object: spicey_tran_kernel_v2
// checks it once) and forms the byte address from the half in ONE instruction, a shift that selects its source half
// (SDWA); reads and writes of the same operand share the register.  A handle is an opaque 32-bit value: the LDS byte
// address in an OA device build, the index itself everywhere else (host code and every other build read W[index * K + k],
// as ever).  index(i): the handle of an index that was computed, not extracted.
template <bool OA>
struct SpiceyOperand {
#if defined(__HIP_DEVICE_COMPILE__)
  static constexpr bool LDS0 = OA;
#else
  static constexpr bool LDS0 = false;
#endif
  template <int H>
  static SPICEY_HD uint32_t half(uint32_t w) {
    static_assert(H == 0 || H == 1, "a word has two halves");
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (LDS0) {
      // (One shift that selects its source half.  hipcc finds it by itself for the upper half, `(w >> 16) << 3`, but with the
      // shift count in a vector register that then stays live around the whole time loop; for the lower half every C++
      // spelling gives a shift and a mask with 0x7fff8.  Written out, the count is an inline constant.  Registers in,
      // register out: nothing else)
      uint32_t a;
      if (H == 1) asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(a) : "v"(w));
      else asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(a) : "v"(w));
      return a;
    }
#endif
    return H ? w >> 16 : w & 0xffffu;
  }
  static SPICEY_HD uint32_t index(uint32_t i) { return LDS0 ? i << 3 : i; }
  template <int K>
  static SPICEY_HD double ld(const double *W, uint32_t a, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (LDS0) {
      static_assert(!OA || K == 1, "operand addresses: one instance per workgroup");
      return *(const double __attribute__((address_space(3))) *)(uintptr_t)a;
    }
#endif
    return W[(size_t)a * K + k];
  }
  template <int K>
  static SPICEY_HD void st(double *W, uint32_t a, int k, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (LDS0) {
      *(double __attribute__((address_space(3))) *)(uintptr_t)a = v;
      return;
    }
#endif
    W[(size_t)a * K + k] = v;
  }
};

// A copy of an argument struct that lives in global memory, through an address the compiler cannot trace back: the fields
// the surrounding code uses are scalar-loaded HERE (s_load, scalar cache), the rest of the copy is dead (see GpuExecV2::fresh).
// On the host (the emulator) it is the struct itself.
template <class X>
SPICEY_HD X spicey_fresh(const X &x) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const X __attribute__((address_space(4))) *cptr;
  cptr p = (cptr)(&x);
  asm volatile("" : "+s"(p));
  X v;
  __builtin_memcpy(&v, p, sizeof(X));
  return v;
#else
  return x;
#endif
}

// 1/x for pivots: hardware reciprocal seed + two Newton steps (<= 1 ulp; the result feeds a 1e-9 parity
// budget, and the reference's own quotient order differs anyway).  The IEEE-exact quotient hipcc emits
// for `1.0 / x` is ~3x longer and sits on the critical path of every factor level.
SPICEY_HD double spicey_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
#else
  return 1.0 / x;
#endif
}

SPICEY_HD double spicey_max_nan(double a, double b) {  // Math.max semantics
  return (a > b || a != a) ? a : b;
}

// ---- exp for the diode model -------------------------------------------------------------------------------------------
// The device library's f64 exp, operation for operation (ROCm device libs, ocml expD.cl as linked into every kernel here):
// n = rint(x log2 e); r = x + n (-ln 2) in two fma steps (ln 2 = hi + lo); a degree-11 polynomial in r, nine Horner steps
// and two closing fma(r, p, 1.0); ldexp(p, n); x > 1024 -> +inf; x < -1075 -> 0.  Same operations on the same constants in
// the same order: the same bits for every argument (NaN and the infinities included; tests/test_u0_resident_gpu.py holds
// a million arguments and the edges against the library).
// Why a copy: inlined into a time loop, the library's exp leaves its literals to the compiler, which keeps all of them —
// nine coefficient pairs, the reduction and clamp constants: 18 .. 24 vector registers — live around the whole loop, in
// kernels that sit at their register cap.  Here the constants come from a table in constant memory through an address the
// compiler cannot trace back (as spicey_fresh reads the argument structs), so they are scalar-loaded inside the phase that
// evaluates a diode and dead behind it: no register, vector or scalar, holds one across the loop.  The diode's own
// literals (0.8, 1e-12) ride in the same table for the same reason.  Who uses it: spicey_diode_k<PORT>.
#define SPICEY_EXP_TAB_VALUES                                                                                                  \
  0x1.71547652b82fep+0,  /* [0] log2 e */                                                                                      \
  -0x1.62e42fefa39efp-1, /* [1] -ln 2, upper part (negated here, as the compiler negates the library's literal: */            \
  -0x1.abc9e3b39803fp-56, /* [2] -ln 2, lower part   fma(-n, c, x) and fma(n, -c, x) differ in the sign of a NaN) */            \
  0x1.ade156a5dcb37p-26, /* [3] .. [11]: the polynomial, highest power first */                                                \
  0x1.28af3fca7ab0cp-22, 0x1.71dee623fde64p-19, 0x1.a01997c89e6b0p-16, 0x1.a01a014761f6ep-13, 0x1.6c16c1852b7b0p-10,         \
  0x1.1111111122322p-7, 0x1.55555555502a1p-5, 0x1.5555555555511p-3, 0x1.000000000000bp-1, /* [12] */                           \
  1024.0,                /* [13] above: +inf */                                                                                \
  -1075.0,               /* [14] below: 0 */                                                                                   \
  0.8,                   /* [15] spicey_diode_k: upper clamp of the junction voltage */                                        \
  1e-12                  /* [16] spicey_diode_k: floor of the conductance */
#define SPICEY_EXP_TAB_N 17
#define SPICEY_EXP_TAB_VHI 15
#define SPICEY_EXP_TAB_GMIN 16
#if defined(__HIP_DEVICE_COMPILE__)
static __device__ __constant__ const double spicey_exp_tab_dev[SPICEY_EXP_TAB_N] = {SPICEY_EXP_TAB_VALUES};
typedef const double __attribute__((address_space(4))) *SpiceyExpTab;
// the table for ONE evaluation site: everything read through the result is loaded behind this point
static __device__ __forceinline__ SpiceyExpTab spicey_exp_tab() {
  SpiceyExpTab t = (SpiceyExpTab)spicey_exp_tab_dev;
  asm volatile("" : "+s"(t));
  return t;
}
#else
typedef const double *SpiceyExpTab;
static inline SpiceyExpTab spicey_exp_tab() {
  static const double tab[SPICEY_EXP_TAB_N] = {SPICEY_EXP_TAB_VALUES};
  return tab;
}
#endif
SPICEY_HD double spicey_exp_port(double x, SpiceyExpTab t) {
  const double dn = __builtin_rint(x * t[0]);
  const double r = __builtin_fma(dn, t[2], __builtin_fma(dn, t[1], x));
  double p = __builtin_fma(r, t[3], t[4]);
  p = __builtin_fma(r, p, t[5]);
  p = __builtin_fma(r, p, t[6]);
  p = __builtin_fma(r, p, t[7]);
  p = __builtin_fma(r, p, t[8]);
  p = __builtin_fma(r, p, t[9]);
  p = __builtin_fma(r, p, t[10]);
  p = __builtin_fma(r, p, t[11]);
  p = __builtin_fma(r, p, t[12]);
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
#if defined(__HIP_DEVICE_COMPILE__)
  double z = __builtin_ldexp(p, (int)dn);
#else
  // (the conversion saturates on the GPU; here an argument outside the int range is one of the two cases below, or NaN)
  double z = __builtin_ldexp(p, (dn > -4096.0 && dn < 4096.0) ? (int)dn : 0);
#endif
  z = x > t[13] ? __builtin_inf() : z;
  z = x < t[14] ? 0.0 : z;
  return z;
}
// exp(x) where a diode is evaluated: the port on the GPU; the host's libm in host builds (the emulators compare against an
// oracle that uses it — spicey_exp_port compiles there too, for the test of the port itself)
SPICEY_HD double spicey_exp(double x, SpiceyExpTab t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return spicey_exp_port(x, t);
#else
  (void)t;
  return exp(x);
#endif
}
SPICEY_HD double spicey_exp(double x) { return spicey_exp(x, spicey_exp_tab()); }

// Diode companion model, simulateTRAN.ts:87-98, and (when `want_i`) the recorded current of :214-217,
// which uses the UNCLAMPED junction voltage.  One exp serves both whenever vd lies inside the clamp
// window [-1, 0.8].  The per-diode constants 1/(N VT) and Is/(N VT) are formed once per evaluation
// from Is, N (two divisions); callers on the hot path pass them precomputed.
// PORT: exp is spicey_exp and the model's own literals come from its table, taken here, once per evaluation — for the
// kernels at their register cap (the fresh packed shape: TranPhases2 asks for it there).  Measured on the MI355X
// (profiles/NOTES_r19.md §5): the kernels with registers to spare lose by it — the table's scalar loads stand in front
// of every evaluation, 2.7 % of a step of the single-instance 1024-thread kernel — so they keep the library's exp and the
// literals, and are compiled exactly as before.  Same bits either way.
template <bool PORT = false>
SPICEY_HD void spicey_diode_k(double vd, double is, double inv_vt, double is_vt, bool want_i, double &gd, double &ieq, double &irec) {
  SpiceyExpTab t = nullptr;
  double vhi = 0.8, gmin = 1e-12;
  if constexpr (PORT) {
    t = spicey_exp_tab();
    vhi = t[SPICEY_EXP_TAB_VHI];
    gmin = t[SPICEY_EXP_TAB_GMIN];
  }
  double vl = vd;
  if (vd > vhi) vl = vhi;
  if (vd < -1.0) vl = -1.0;
  const double e = PORT ? spicey_exp(vl * inv_vt, t) : exp(vl * inv_vt);
  const double id = is * (e - 1.0);
  gd = spicey_max_nan(is_vt * e, gmin);
  ieq = id - gd * vl;
  irec = id;
  if (want_i && vl != vd) irec = is * ((PORT ? spicey_exp(vd * inv_vt, t) : exp(vd * inv_vt)) - 1.0);
}
SPICEY_HD void spicey_diode(double vd, double is, double nn, double &gd, double &ieq) {
  const double vt = nn * SPICEY_VT300;
  double irec;
  spicey_diode_k(vd, is, 1.0 / vt, is / vt, false, gd, ieq, irec);
}

SPICEY_HD double spicey_switch_g(int on, double ron, double roff) {  // simulateTRAN.ts:59-61
  const double r = on ? ron : roff;
  return 1.0 / spicey_max_nan(fabs(r), SPICEY_EPS);
}
