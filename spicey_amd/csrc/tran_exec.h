// tran_exec.h — the per-workgroup transient program interpreter (device code, host-compilable).
//
// One workgroup owns K instances (same topology, interleaved [index][K] in LDS) and runs the whole
// `for step … for iter …` nest of /root/reference/lib/analysis/simulateTRAN.ts:146-238 for them
// inside ONE kernel launch.  Every function below is the body of one barrier-separated PHASE;
// inside a phase the threads are independent (gather form: each thread owns what it writes, reads
// only data finalised in earlier phases), so the same code can be
//   * the HIP kernel (kernels.hip): `phase(f)` = f(threadIdx.x); __syncthreads();
//   * the CPU test emulator (tests/emul): `phase(f)` = for tid in 0..T-1: f(tid)
// The emulator is test infrastructure for the symbolic phase and this interpreter; the product
// path only ever runs the HIP kernel.
//
// Phases per time step (nLev = elimination-tree height):
//   B    dynamic stamps (switch / diode conductances) + right-hand side          simulateTRAN.ts:25-102
//   U_l  l = 0..nLev-2: Schur updates of level l with the forward elimination fused in as an extra
//        column; diagonals that become final are stored as reciprocals (singularity check = solveReal.ts:28)
//   K_l  l = nLev-1..0: backward substitution                                    solveReal.ts:56-72
//   S    switch hysteresis + iteration control (only if the circuit has switches) simulateTRAN.ts:108-128,151-162
//   Z    recording, state update, and the NEXT step's element evaluation          simulateTRAN.ts:164-237
//
// The code lives in the pieces below, by layer; each includes what it uses, top to bottom:
//   tran_common.h     SPICEY_HD, device / host macro pairs, phase tags, WgCtx, spicey_fresh, element models
//   tran_pt_layout.h  where the phase table and the operand slots lie, which step counts the ready arguments take (plain arithmetic: the launch plan reads it too)
//   tran_pt.h         the phase table (run-invariant phase arguments in LDS)          <- common, pt_layout
//   tran_v1_phases.h  diagnostics, TranPhases<K>                                      <- common
//   tran_rec16.h      ResRegs, the 16-bit record interpreter, spicey_uk_phase         <- common, pt
//   tran_v2_phases.h  TranPhases2                                                     <- all of the above
//   tran_v2_run.h     the tridiagonal top (spicey_pcr_*), spicey_tran_run_v2          <- all of the above
//   tran_v1_run.h     spicey_tran_run, fronts_exec.h                                  <- v1 phases, fronts_exec.h
#pragma once
#include "tran_common.h"
#include "tran_pt.h"
#include "tran_v1_phases.h"
#include "tran_rec16.h"
#include "tran_v2_phases.h"
#include "tran_v2_run.h"
#include "tran_v1_run.h"
