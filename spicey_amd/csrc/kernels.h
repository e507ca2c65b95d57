// kernels.h — host-callable launchers of kernels.hip, exact.hip, ac.hip and ac_exact.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include "devbuf.h"
#include "launch_plan.h"
#include "program.h"

#define SPICEY_GRP_SYNC_WORDS 320  // uint32 words of barrier state per group: [0] flat counter, [1] abort, [2..7] timeout note, [8] stale polls, [16..] XCD census / arrivals / top / generation

hipError_t spicey_launch_tran(const SpiceyProg &P, const SpiceyRun &R, int K, bool lds, int grid, int threads, hipStream_t st);

// v2 (register-resident program): one kernel per build of SPICEY_V2_SHAPES (launch_plan.h), K = 1 only
// (Ph / Qh: host copies for the launch geometry; P / Q / R: the same structs in DEVICE memory — the kernel reads them by scalar loads;
// phase_table: take the build that keeps its run-invariant phase arguments in LDS where the program has room for them, tran_exec.h;
// early: R->zpar is set — take the shape's early-prefetch kernel, an error where it has none;
// slots: LaunchPlan::slots — take the shape's operand-slot kernel, an error without `early`, the table or room for the slots;
// ready: LaunchPlan::ready and spicey_ready_steps_ok(steps of this run) — its ready-argument form, an error without `slots`;
// addr: spicey_addr_run — that form with operand addresses, an error without `ready` or where spicey_addr_fits does not hold;
// top_regs: spicey_top_regs_run — that form with the register-exchange top, an error without `addr` or for a top outside 1 .. 6 stages;
// u0_resident: spicey_u0_resident_run — that form with the resident level-0 record, an error without `top_regs`;
// top_fold: spicey_top_fold_run and the record table stands behind R->zpar — that form with the last factor level folded into the top, an error without `u0_resident`;
// fixed_schedule: spicey_fixed_schedule_run — the fused kernel with the time loop written out, an error without `stamp_fuse`; profile: the handle asked for
// phase timers — that form's kernel with the profiling executor instead of the production one (every other form has one kernel for both);
// stamp_fuse: spicey_stamp_fuse_run and that form's table stands behind the fold's — the folded kernel whose Z stamps the next step, an error without `top_fold`)
hipError_t spicey_launch_tran_v2(const SpiceyProg &Ph, const SpiceyResident &Qh, const SpiceyProg *P, const SpiceyResident *Q, const SpiceyRun *R, int K, int grid,
                                 int threads, hipStream_t st, bool packed = false, bool phase_table = true, bool early = false, bool slots = false, bool ready = false, bool addr = false, bool top_regs = false, bool u0_resident = false, bool top_fold = false, bool stamp_fuse = false, bool fixed_schedule = false, bool profile = false);

// group mode: R.wgs_per_group workgroups per K instances, workspace in global memory (large circuits)
hipError_t spicey_launch_tran_grp(const SpiceyProg &P, const SpiceyRun &R, int K, int n_groups, int threads, hipStream_t st);
int spicey_grp_blocks_per_cu(const SpiceyProg &P, int K, int threads);  // occupancy of that kernel (0: cannot run)

// reference-order engine (exact.hip): one workgroup per instance; P, R in DEVICE memory; lds = dynamic LDS bytes, 0 = the
// workspace is R->gW
struct SpiceyExactProg;
hipError_t spicey_launch_exact(const SpiceyExactProg *P, const SpiceyRun *R, int grid, int threads, size_t lds, hipStream_t st);

// AC sweep (ac.hip), one workgroup per (instance, frequency) slot from R.slot_base on: lds_bytes = dynamic LDS of the
// workspace, 0 = each workgroup's slice of R.gW
struct SpiceyAcRun;
struct SpiceyCx;
hipError_t spicey_launch_ac(const SpiceyProg &P, const SpiceyAcRun &R, int grid, int threads, size_t lds_bytes, hipStream_t st);
// resident sweep: n_inst * n_chunk workgroups of <= 512 threads, each running frequencies c, c + n_chunk, ... of its instance
// with SPICEY_AC_RMAX task records and the stamp parts of SPICEY_AC_NSE entries per thread in registers (256 VGPRs, no spills)
#define SPICEY_AC_RMAX 12
#define SPICEY_AC_NSE 10
hipError_t spicey_launch_ac_resident(const SpiceyProg &P, const SpiceyResident &Q, const SpiceyAcRun &R, int n_chunk, int threads, size_t lds_bytes, hipStream_t st);
// dense partial-pivoting re-solve of the `count` slots listed in d_slots (P, R in DEVICE memory; n = P->n): Ws [count][nW]
// sparse scratch, A [count][n (n + 1)]
hipError_t spicey_launch_ac_dense(const SpiceyProg *P, const SpiceyAcRun *R, int n, const int64_t *d_slots, int count, SpiceyCx *Ws, SpiceyCx *A, hipStream_t st);

// reference-order AC engine (ac_exact.hip): one workgroup per (instance, frequency) slot from slot_base on; P, R in DEVICE
// memory; lds = dynamic LDS bytes, 0 = the workspace is R->gW
struct SpiceyAcExactProg;
struct SpiceyAcExactRun;
hipError_t spicey_launch_ac_exact(const SpiceyAcExactProg *P, const SpiceyAcExactRun *R, int64_t slot_base, int grid, int threads, size_t lds, hipStream_t st);
