// tran_pt_layout.h — where the phase table and the operand slots lie in the tail area (tran_pt.h has the table itself).
// Plain integer arithmetic on SpiceyProg's fields, free of device intrinsics: the launch plan includes it as well as the kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "program.h"

#if defined(__HIPCC__)
#define SPICEY_LAYOUT_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define SPICEY_LAYOUT_FN inline
#endif
#define SPICEY_PT_RUN 48  // 32-bit words of the table's run-wide block (tran_pt.h)
SPICEY_LAYOUT_FN int spicey_pt_base_words(int pcr_n) { return 1024 + ((pcr_n * 2 + 3) & ~3); }
// rows of the table of a program with its top at level `pcr_level`, and whether they fit behind the top's index table
SPICEY_LAYOUT_FN int spicey_pt_words(int pcr_level) { return SPICEY_PT_RUN + 16 * pcr_level; }
SPICEY_LAYOUT_FN bool spicey_pt_fits(int pcr_n, int pcr_level, int tail_n) {
  // (a phase head reads 64 consecutive words from the start of the table, SpiceyPtLanes: with pcr_level >= 1 they lie inside it)
  return pcr_n > 0 && pcr_n <= 64 && pcr_level >= 1 && tail_n == 0 && spicey_pt_base_words(pcr_n) + spicey_pt_words(pcr_level) <= 5 * 256;
}
// ---- operand slots (operand-slot builds, tran_v2_run.h: OS) ---------------------------------------------------------------
// Two read-only doubles, written by the prologue and never again: +0.0, which a ground terminal reads instead of being
// compared and masked (v - (+0.0) and (+0.0) - v are what TranPhases2::dv16 computes, signs of zero included), and -0.0
// behind it, the neutral element of an addition (x + (-0.0) == x for every x, both zeros included).  They take the last
// four words of the 5 KB tail area of a tridiagonal-top build, behind the phase table, and are addressed like any other
// operand: by their index from the start of the LDS workspace (K = 1, LDS layout of spicey_lds_bytes: the workspace, the
// switch states and flags, the profiling slots, then the tail area).  A program whose table leaves no room there, or whose
// slots a 16-bit index from the start of the workspace, or a 14-bit one from the start of the element vectors (phase B's
// descriptor fields: TranPhases2::dd_slots / rhs_slots), cannot reach, keeps the builds without them (spicey_plan).
#define SPICEY_SLOT_TAIL_WORD (5 * 256 - 4)
SPICEY_LAYOUT_FN uint32_t spicey_slot_index(const SpiceyProg &P) {  // of +0.0; -0.0 is the next double
  const size_t ws = ((size_t)P.nW + (size_t)P.nU + (size_t)P.nGdyn) * sizeof(double) + ((size_t)P.nS + 4) * sizeof(int32_t);
  const size_t tail = ((ws + 15) & ~(size_t)15) + SPICEY_PH_SLOTS * sizeof(unsigned long long);
  return (uint32_t)((tail + (size_t)SPICEY_SLOT_TAIL_WORD * 4) / sizeof(double));
}
SPICEY_LAYOUT_FN bool spicey_slots_fit(const SpiceyProg &P, int tail_n) {
  return !P.hybrid && spicey_pt_fits(P.pcr_n, P.pcr_level, tail_n) && spicey_pt_base_words(P.pcr_n) + spicey_pt_words(P.pcr_level) <= SPICEY_SLOT_TAIL_WORD &&
         spicey_slot_index(P) + 1 < 0xFFFFu && spicey_slot_index(P) + 1 - (uint32_t)P.nW <= 0x3FFFu;
}
// ---- ready arguments (ready-argument builds, tran_v2_run.h: RA) -----------------------------------------------------------
// Such a build forms the per-step offsets step x nOut, step x nCur and (step + 1) x nV as ONE 32 x 32 -> 64-bit product of
// the low words.  The row sizes are non-negative 32-bit counts; the product is exact as long as step + 1 fits 32 bits for
// every step of the run, that is steps <= 2^32 - 2.  The step count is known per run, not per handle: the launch checks
// it (spicey_abi.cpp: enqueue_kernel) and a run outside the condition takes the operand-slot kernel without ready arguments.
#define SPICEY_READY_MAX_STEPS 0xFFFFFFFEll
SPICEY_LAYOUT_FN bool spicey_ready_steps_ok(int64_t steps) { return steps >= 0 && steps <= SPICEY_READY_MAX_STEPS; }
// ---- the parameter record and the fold's table behind it (tran_v2_run.h: EP, TF) ------------------------------------------
// SpiceyRun::zpar holds five doubles per resident item, NEL x T items per instance; a run that folds the last factor level
// into the top keeps that form's record table — SPICEY_TOP_FOLD_WORDS 32-bit words: 64 records of 8, the top's first 2 KB row
// buffer — right behind them in the same allocation.  Host (allocation, upload) and kernel (prologue) both take the record's
// size from here.
#define SPICEY_TOP_FOLD_WORDS 512
SPICEY_LAYOUT_FN size_t spicey_zpar_record_doubles(int n_inst, int nel, int threads) { return (size_t)n_inst * (size_t)nel * (size_t)threads * 5; }
// ---- the stamp fuse's table (tran_v2_run.h: SF), behind the fold's ----------------------------------------------------------
// A run whose Z stamps the next step keeps that form's table — six 32-bit words per thread: its two entry slots, its two
// row slots, the row of its source, one unused (launch_plan.h: spicey_stamp_fuse_table has the fields) — right behind the
// fold's table, in the same allocation.  Topology only: one table for all instances.
#define SPICEY_STAMP_FUSE_THREAD_WORDS 6
#define SPICEY_SF_NONE 0x80000000u   // the slot holds nothing: nothing is written
#define SPICEY_SF_RECIP 0x40000000u  // entry slot: the reciprocal is stored, and the pivot is held against SPICEY_EPS
#define SPICEY_SF_F0 0x00010000u     // first operand present (entry: the entry's first field, + gd; row: gc v of the capacitor)
#define SPICEY_SF_F0_NEG 0x00020000u // ... and subtracted
#define SPICEY_SF_F1 0x00040000u     // second operand present (entry: the second field, + gd; row: ieq of the diode)
#define SPICEY_SF_F1_NEG 0x00080000u // ... and subtracted
#define SPICEY_SF_SWAP 0x00100000u   // row slot: the diode's field stands in front of the capacitor's
SPICEY_LAYOUT_FN size_t spicey_stamp_fuse_words(int threads) { return (size_t)threads * SPICEY_STAMP_FUSE_THREAD_WORDS; }
// ---- operand addresses (operand-address builds, tran_v2_run.h: OA) ---------------------------------------------------------
// Such a build takes c.W for LDS address 0 (K = 1, LDS workspace, no hybrid layout: the dynamic array is the kernel's only
// LDS object) and re-encodes the fields of B's resident descriptors — 14 bits each, indices into c.gd / c.u in the
// operand-slot build — as indices from the start of W (TranPhases2::dd_addr / rhs_addr).  The largest index any field then
// names is the -0.0 slot's, spicey_slot_index + 1, in dd and rhs alike: 14 bits must hold it.  A program beyond that keeps
// the ready-argument kernel without operand addresses (spicey_plan).
#define SPICEY_ADDR_FIELD_MAX 0x3FFFu
SPICEY_LAYOUT_FN uint32_t spicey_addr_max_index(const SpiceyProg &P) { return spicey_slot_index(P) + 1u; }
SPICEY_LAYOUT_FN bool spicey_addr_fits(const SpiceyProg &P, int tail_n) {
  return !P.hybrid && spicey_slots_fit(P, tail_n) && spicey_addr_max_index(P) <= SPICEY_ADDR_FIELD_MAX;
}
