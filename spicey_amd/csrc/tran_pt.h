// tran_pt.h — the phase table: layout, lane access, and the prologue that builds it (tran_exec.h is the map).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "program.h"
#include "tran_common.h"
#include "tran_pt_layout.h"

// ---- run-invariant phase arguments, kept on chip (16-bit interpreter, K = 1, tridiagonal-top builds) -------------------
// What a phase of the time loop needs from SpiceyProg / SpiceyResident / SpiceyRun never changes during a run, yet every
// phase of every step used to fetch it again through scalar loads.  Where those loads were CHAINED they stood exposed in
// front of the phase's first work: three dependent round trips in front of a streamed phase's first record, two in front
// of Z's parameter fetch, three and four at the heads of B and Z (profiles/NOTES_r04.md).  The prologue now writes the
// values ONCE into a table in LDS.  A phase head reads them with one ds_read_b32 — lane l reads word l — and moves each
// word to a scalar by v_readlane (SpiceyPtLanes); the rare reads inside divergent code are same-address broadcast reads.
// The table lives in space that is reserved already: the tail area of a tridiagonal-top build is 5 KB (launch_plan.cpp),
// of which the two row buffers take 4 KB and the top's index table pcr_n * 8 <= 512 B.  Layout, in 32-bit words from
// c.tail + 1024 + (pcr_n * 2 rounded up to 4): SPICEY_PT_RUN run-wide words (below), then one 8-word row per phase that
// can be streamed — the factor phases [0, pcr_level) and the backward phases [2 nLevels - pcr_level, 2 nLevels) — holding
// that phase's SpiceyResident::st_desc row.  A program whose rows do not fit (deep elimination trees), one without a top
// (its tail area is full of tail records) or a handle created with SPICEY_NO_PHASE_TABLE set keeps the scalar loads: both paths
// are compiled and give identical bits (same operands, same order; only addresses and counts come from elsewhere).
enum {
  SPICEY_PT_XOFF = 0, SPICEY_PT_NRESTORE, SPICEY_PT_NDYNENT, SPICEY_PT_NGSTAT, SPICEY_PT_NR, SPICEY_PT_NC, SPICEY_PT_NL, SPICEY_PT_NV,
  // 64-bit values, two words each.  (Words 8..13: what a streamed phase needs beside its row — SpiceyPtLanes::row.)
  SPICEY_PT_OVF16 = 8, SPICEY_PT_REC16 = 10, SPICEY_PT_FUS16 = 12,
  SPICEY_PT_NS = 14, SPICEY_PT_ND, SPICEY_PT_NOUT, SPICEY_PT_NCUR,
  SPICEY_PT_STEPS = 18, SPICEY_PT_SRC = 20, SPICEY_PT_SRC_STRIDE = 22, SPICEY_PT_OUT_V = 24, SPICEY_PT_OUT_I = 26, SPICEY_PT_GSTAT = 28,  // (OUT_V, OUT_I in an operand-slot build: spicey_pt_rebase_rows)
  SPICEY_PT_DPAR = 30, SPICEY_PT_D_IS = 32, SPICEY_PT_C_VPREV = 34, SPICEY_PT_D_VDPREV = 36, SPICEY_PT_ITERS = 38, SPICEY_PT_LIN_VD = 40,
  SPICEY_PT_LIN_ERR = 42,
  SPICEY_PT_USED = 44,
  // early-prefetch builds only (spicey_pt_build's `ep`): SpiceyRun::zpar in two of the four words left of the block; every
  // other build writes and reads the block up to SPICEY_PT_USED, as before
  SPICEY_PT_ZPAR = 44,
  SPICEY_PT_USED_EP = 46
};
static_assert(SPICEY_PT_USED <= SPICEY_PT_ZPAR && SPICEY_PT_USED_EP <= SPICEY_PT_RUN && SPICEY_PT_RUN <= 64 && SPICEY_PT_RUN % 4 == 0, "run-wide block of the phase table: at most one word per lane of a wave");
SPICEY_HD uint32_t spicey_pt_u32(const uint32_t *pt, int i) { return (uint32_t)SPICEY_UNIFORM((int)pt[i]); }
SPICEY_HD uint64_t spicey_pt_u64(const uint32_t *pt, int i) { return (uint64_t)spicey_pt_u32(pt, i) | ((uint64_t)spicey_pt_u32(pt, i + 1) << 32); }
template <class X>
SPICEY_HD X *spicey_pt_ptr(const uint32_t *pt, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef X __attribute__((address_space(1))) *gptr;  // (a global-memory pointer: accesses through it stay global_load / global_store, not flat)
  return (X *)(gptr)(uintptr_t)spicey_pt_u64(pt, i);
#else
  return (X *)(uintptr_t)spicey_pt_u64(pt, i);
#endif
}
// (a 64-bit value as a pointer into global memory, the way spicey_pt_ptr makes one of two words)
template <class X>
SPICEY_HD X *spicey_global_ptr(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef X __attribute__((address_space(1))) *gptr;
  return (X *)(gptr)(uintptr_t)v;
#else
  return (X *)(uintptr_t)v;
#endif
}
SPICEY_HD void spicey_pt_put64(uint32_t *pt, int i, uint64_t v) { pt[i] = (uint32_t)v; pt[i + 1] = (uint32_t)(v >> 32); }
// (the three above: one word, read by every ACTIVE lane from the same address — for the rare reads inside divergent code)
// Many words at a phase head, where the whole wave is active: lane l reads word l — ONE ds_read_b32, one vector register —
// and each word goes to a scalar by v_readlane at a constant lane.  (Broadcast reads would hold a vector register per
// word until it has been moved: the 128-register builds have none to give.)
struct SpiceyPtLanes {
#if defined(__HIP_DEVICE_COMPILE__)
  int v;
  __device__ __forceinline__ uint32_t u32(int i) const { return (uint32_t)__builtin_amdgcn_readlane(v, i); }
#else
  const uint32_t *run, *rowp;
  uint32_t u32(int i) const { return (rowp && i < 8) ? rowp[i] : run[i]; }
#endif
  SPICEY_HD uint64_t u64(int i) const { return (uint64_t)u32(i) | ((uint64_t)u32(i + 1) << 32); }
  template <class X>
  SPICEY_HD X *ptr(int i) const {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef X __attribute__((address_space(1))) *gptr;
    return (X *)(gptr)(uintptr_t)u64(i);
#else
    return (X *)(uintptr_t)u64(i);
#endif
  }
  // the run-wide block
  static SPICEY_HD SpiceyPtLanes run_block(const uint32_t *pt, int tid) {
#if defined(__HIP_DEVICE_COMPILE__)
    return SpiceyPtLanes{(int)pt[tid & 63]};
#else
    (void)tid;
    return SpiceyPtLanes{pt, nullptr};
#endif
  }
  // words 0..7 = row `row` of the per-phase rows, words 8.. = the run-wide block's
  static SPICEY_HD SpiceyPtLanes row(const uint32_t *pt, int tid, int row) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int l = tid & 63;
    return SpiceyPtLanes{(int)pt[l < 8 ? SPICEY_PT_RUN + row * 8 + l : l]};
#else
    (void)tid;
    return SpiceyPtLanes{pt, pt + SPICEY_PT_RUN + row * 8};
#endif
  }
};

// ---- the phase table (see the top of this file) ---------------------------------------------------------------------------
// Whether a run keeps one is decided on the host.  The GPU kernels are built twice, with the table (PT = 1) and with the
// scalar loads (PT = 0) — one kernel holding both paths of B and Z does not fit the 128 registers of the two-workgroups-
// per-CU build —, and spicey_launch_tran_v2 picks the build: spicey_pt_fits and no SPICEY_NO_PHASE_TABLE in the
// environment of spicey_create.  PT = -1 (the test emulator, which instantiates the interpreter itself) decides per run:
SPICEY_HD bool spicey_pt_runtime_choice(const SpiceyProg &P, const SpiceyResident &Q) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)P; (void)Q;
  return false;
#else
  return spicey_pt_fits(P.pcr_n, P.pcr_level, Q.tail_n) && getenv("SPICEY_NO_PHASE_TABLE") == nullptr;
#endif
}
// Written once, in the prologue.  Every word of the run-wide block is a 32-bit piece of one field of SpiceyProg or
// SpiceyRun: lane l copies word l from where the struct lives (a vector load: no scalar registers, which the prologue
// phase that fills the resident registers has none to spare of either).
struct SpiceyPtWord {
  uint16_t from_run;  // 0: SpiceyProg, 1: SpiceyRun
  uint16_t off;       // byte offset of the word
};
#define SPICEY_PT_P32(f) {0, (uint16_t)offsetof(SpiceyProg, f)}
#define SPICEY_PT_P64(f) {0, (uint16_t)offsetof(SpiceyProg, f)}, {0, (uint16_t)(offsetof(SpiceyProg, f) + 4)}
#define SPICEY_PT_R64(f) {1, (uint16_t)offsetof(SpiceyRun, f)}, {1, (uint16_t)(offsetof(SpiceyRun, f) + 4)}
template <int K>
SPICEY_HD void spicey_pt_build(const SpiceyProg &P, const SpiceyResident &Q, const SpiceyRun &R, const WgCtx<K> &c, int tid, int T, bool ep = false) {
  static constexpr SpiceyPtWord words[SPICEY_PT_USED] = {
      SPICEY_PT_P32(xoff), SPICEY_PT_P32(nRestore), SPICEY_PT_P32(nDynEnt), SPICEY_PT_P32(nGstat), SPICEY_PT_P32(nR), SPICEY_PT_P32(nC),
      SPICEY_PT_P32(nL), SPICEY_PT_P32(nV), SPICEY_PT_P64(ovf16), SPICEY_PT_P64(rec16), SPICEY_PT_P64(fus16), SPICEY_PT_P32(nS),
      SPICEY_PT_P32(nD), SPICEY_PT_P32(nOut), SPICEY_PT_P32(nCur), SPICEY_PT_R64(steps), SPICEY_PT_R64(src), SPICEY_PT_R64(src_stride),
      SPICEY_PT_R64(out_v), SPICEY_PT_R64(out_i), SPICEY_PT_R64(gstat), SPICEY_PT_R64(dpar), SPICEY_PT_R64(D_is), SPICEY_PT_R64(C_vprev),
      SPICEY_PT_R64(D_vdprev), SPICEY_PT_R64(iters), SPICEY_PT_R64(lin_vd), SPICEY_PT_R64(lin_err)};
  uint32_t *pt = c.tail + spicey_pt_base_words(P.pcr_n);
  if (tid < SPICEY_PT_USED) {
    const SpiceyPtWord w = words[tid];
    const char *src = (w.from_run ? (const char *)&R : (const char *)&P) + w.off;
    uint32_t v;
    __builtin_memcpy(&v, src, 4);
    pt[tid] = v;
  }
  if (ep && tid >= SPICEY_PT_ZPAR && tid < SPICEY_PT_USED_EP) {  // (`ep`: a constant of the build)
    uint32_t v;
    __builtin_memcpy(&v, (const char *)&R + offsetof(SpiceyRun, zpar) + (size_t)(tid - SPICEY_PT_ZPAR) * 4, 4);
    pt[tid] = v;
  }
  const int L = P.pcr_level, kb = 2 * P.nLevels - L;  // rows: factor phases [0, L), then backward phases [kb, kb + L)
  for (int i = tid; i < 2 * L * 8; i += T) {
    const int r = i >> 3, p = r < L ? r : kb + (r - L);
    pt[SPICEY_PT_RUN + i] = Q.st_desc[(size_t)p * 8 + (i & 7)];
  }
}
// Operand-slot builds, behind spicey_pt_build in the same phase (thread `tid` wrote word `tid` there): the two result pointers
// become those of row 0 of THIS workgroup's instance, so that Z adds only step x row per step instead of multiplying
// (inst (steps + 1) + step) x row out in 64-bit scalars.  A null current pointer stays null.
template <int K>
SPICEY_HD void spicey_pt_rebase_rows(const SpiceyProg &P, const SpiceyRun &R, const WgCtx<K> &c, int tid) {
  static_assert(SPICEY_PT_OUT_I == SPICEY_PT_OUT_V + 2 && SPICEY_PT_OUT_V % 2 == 0, "the two result pointers are neighbours in the table");
  if (tid < SPICEY_PT_OUT_V || tid >= SPICEY_PT_OUT_I + 2) return;
  const bool cur = tid >= SPICEY_PT_OUT_I;
  const double *b = cur ? R.out_i : R.out_v;
  const uint64_t a = b ? (uint64_t)(uintptr_t)(b + (size_t)c.inst[0] * (size_t)(R.steps + 1) * (size_t)(cur ? P.nCur : P.nOut)) : 0u;
  (c.tail + spicey_pt_base_words(P.pcr_n))[tid] = (uint32_t)(a >> (32 * (tid & 1)));
}
// Ready-argument builds (tran_v2_run.h: RA), behind the two above in the same phase: three more pointers become those of THIS
// workgroup's instance, so that no phase multiplies the instance's share out again in 64-bit scalars —
//   SPICEY_PT_ZPAR   the instance's parameter record, zpar + inst x `zrec` doubles (zrec = NEL x T x 5: TranPhases2::zpar_fill)
//   SPICEY_PT_SRC    the instance's source table, src + inst x src_stride
//   SPICEY_PT_ITERS  the instance's row of iteration counts, iters + inst x (steps + 1)
// A null pointer stays null.  Only the hot readers below (spicey_pt_args_z / spicey_pt_args_early) and the lazy reads of
// the same build see these words; what a cold branch takes from the complete structs in global memory is what it was.
template <int K>
SPICEY_HD void spicey_pt_rebase_ready(const SpiceyProg &P, const SpiceyRun &R, const WgCtx<K> &c, int tid, size_t zrec) {
  static_assert(SPICEY_PT_ZPAR % 2 == 0 && SPICEY_PT_SRC % 2 == 0 && SPICEY_PT_ITERS % 2 == 0, "64-bit words of the table start at even indices");
  const int w = tid & ~1;
  if (w != SPICEY_PT_ZPAR && w != SPICEY_PT_SRC && w != SPICEY_PT_ITERS) return;
  const size_t in = (size_t)c.inst[0];
  uint64_t a;
  if (w == SPICEY_PT_ZPAR) a = R.zpar ? (uint64_t)(uintptr_t)(R.zpar + in * zrec) : 0u;
  else if (w == SPICEY_PT_SRC) a = R.src ? (uint64_t)(uintptr_t)(R.src + in * (size_t)R.src_stride) : 0u;
  else a = R.iters ? (uint64_t)(uintptr_t)(R.iters + in * (size_t)(R.steps + 1)) : 0u;
  (c.tail + spicey_pt_base_words(P.pcr_n))[tid] = (uint32_t)(a >> (32 * (tid & 1)));
}
// ... and what the always-executed code of these builds moves to scalars at a phase head.  Z (TranPhases2::z_record): the
// four counts that bound resident items, nV / nL / nS, the width of a current row, the two row-0 result pointers and
// the instance's iteration counts; whether this is the last step comes from the run loop's own scalars.  Everything else
// that Z may touch — the end-state arrays of the last step, the record and the source table where nothing was
// prefetched — is read where it is used, inside its branch (spicey_pt_ptr), and the beyond-capacity loops take the
// complete structs as before.
SPICEY_HD void spicey_pt_args_z(const SpiceyPtLanes &a, SpiceyProg &P, SpiceyRun &R) {
  P.nR = (int32_t)a.u32(SPICEY_PT_NR); P.nC = (int32_t)a.u32(SPICEY_PT_NC); P.nD = (int32_t)a.u32(SPICEY_PT_ND); P.nOut = (int32_t)a.u32(SPICEY_PT_NOUT);
  P.nV = (int32_t)a.u32(SPICEY_PT_NV); P.nL = (int32_t)a.u32(SPICEY_PT_NL); P.nS = (int32_t)a.u32(SPICEY_PT_NS); P.nCur = (int32_t)a.u32(SPICEY_PT_NCUR);
  R.out_v = a.template ptr<double>(SPICEY_PT_OUT_V);
  R.out_i = a.template ptr<double>(SPICEY_PT_OUT_I);
  R.iters = a.template ptr<int32_t>(SPICEY_PT_ITERS);
}
// The early fetch (TranPhases2::z_early): the number of sources, the instance's record and its source table.
SPICEY_HD void spicey_pt_args_early(const SpiceyPtLanes &a, SpiceyProg &P, SpiceyRun &R) {
  P.nV = (int32_t)a.u32(SPICEY_PT_NV);
  R.src = a.template ptr<const double>(SPICEY_PT_SRC);
  R.zpar = a.template ptr<double>(SPICEY_PT_ZPAR);
}
// The fields that the always-executed code of B, Z and Z's parameter prefetch reads (TranPhases2, K = 1, LDS workspace), from
// the table into two LOCAL structs; every other field stays zero and is never looked at there (TranPhases2::Pg).  What a
// phase does not use of this is dead code.
SPICEY_HD void spicey_pt_args(const uint32_t *pt, int tid, SpiceyProg &P, SpiceyRun &R) {
  const SpiceyPtLanes a = SpiceyPtLanes::run_block(pt, tid);  // (called at a phase head: the whole wave is here)
  P.xoff = (int32_t)a.u32(SPICEY_PT_XOFF); P.nRestore = (int32_t)a.u32(SPICEY_PT_NRESTORE);
  P.nDynEnt = (int32_t)a.u32(SPICEY_PT_NDYNENT); P.nGstat = (int32_t)a.u32(SPICEY_PT_NGSTAT);
  P.nR = (int32_t)a.u32(SPICEY_PT_NR); P.nC = (int32_t)a.u32(SPICEY_PT_NC); P.nL = (int32_t)a.u32(SPICEY_PT_NL);
  P.nV = (int32_t)a.u32(SPICEY_PT_NV); P.nS = (int32_t)a.u32(SPICEY_PT_NS); P.nD = (int32_t)a.u32(SPICEY_PT_ND);
  P.nOut = (int32_t)a.u32(SPICEY_PT_NOUT); P.nCur = (int32_t)a.u32(SPICEY_PT_NCUR);
  R.steps = (int64_t)a.u64(SPICEY_PT_STEPS);
  R.src = a.template ptr<const double>(SPICEY_PT_SRC);
  R.src_stride = (int64_t)a.u64(SPICEY_PT_SRC_STRIDE);
  R.out_v = a.template ptr<double>(SPICEY_PT_OUT_V);
  R.out_i = a.template ptr<double>(SPICEY_PT_OUT_I);
  R.gstat = a.template ptr<double>(SPICEY_PT_GSTAT);
  R.dpar = a.template ptr<double>(SPICEY_PT_DPAR);
  R.D_is = a.template ptr<const double>(SPICEY_PT_D_IS);
  R.C_vprev = a.template ptr<double>(SPICEY_PT_C_VPREV);
  R.D_vdprev = a.template ptr<double>(SPICEY_PT_D_VDPREV);
  R.iters = a.template ptr<int32_t>(SPICEY_PT_ITERS);
  R.lin_vd = a.template ptr<double>(SPICEY_PT_LIN_VD);
  R.lin_err = a.template ptr<unsigned long long>(SPICEY_PT_LIN_ERR);
  R.zpar = a.template ptr<double>(SPICEY_PT_ZPAR);  // (read by the early-prefetch builds only, which write the word)
}
