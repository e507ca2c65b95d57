// kernels.h — host-callable launchers of kernels.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include "launch_plan.h"
#include "program.h"

#define SPICEY_GRP_SYNC_WORDS 320  // uint32 words of barrier state per group: [0] flat counter, [1] abort, [2..7] timeout note, [8] stale polls, [16..] XCD census / arrivals / top / generation

hipError_t spicey_launch_tran(const SpiceyProg &P, const SpiceyRun &R, int K, bool lds, int grid, int threads, hipStream_t st);

// v2 (register-resident program): one kernel per build of SPICEY_V2_SHAPES (launch_plan.h), K = 1 only
// (Ph / Qh: host copies for the launch geometry; P / Q / R: the same structs in DEVICE memory — the kernel reads them by scalar loads;
// phase_table: take the build that keeps its run-invariant phase arguments in LDS where the program has room for them, tran_exec.h)
hipError_t spicey_launch_tran_v2(const SpiceyProg &Ph, const SpiceyResident &Qh, const SpiceyProg *P, const SpiceyResident *Q, const SpiceyRun *R, int K, int grid,
                                 int threads, hipStream_t st, bool packed = false, bool phase_table = true);

// group mode: R.wgs_per_group workgroups per K instances, workspace in global memory (large circuits)
hipError_t spicey_launch_tran_grp(const SpiceyProg &P, const SpiceyRun &R, int K, int n_groups, int threads, hipStream_t st);
int spicey_grp_blocks_per_cu(const SpiceyProg &P, int K, int threads);  // occupancy of that kernel (0: cannot run)

// reference-order engine (exact.hip): one workgroup per instance; P, R in DEVICE memory; lds = dynamic LDS bytes, 0 = the
// workspace is R->gW
struct SpiceyExactProg;
hipError_t spicey_launch_exact(const SpiceyExactProg *P, const SpiceyRun *R, int grid, int threads, size_t lds, hipStream_t st);

// reference-order AC engine (ac_exact.hip): one workgroup per (instance, frequency) slot.  The spicey_ac_* entry points of
// ac.hip hand a handle created with SpiceyOptions.interpreter = 3 to these; `err` / spicey_ac_exact_error carry the message.
struct SpiceyAcExact;
int32_t spicey_ac_exact_create(const SpiceyDesc *desc, const SpiceyOptions &opt, SpiceyAcExact **out, std::string &err);
struct SpiceyAcSweep;
int32_t spicey_ac_exact_sweep(SpiceyAcExact *x, int64_t n_freq, const double *freqs, const double *vph, bool want_i, SpiceyAcSweep &o, double *ms);
hipStream_t spicey_ac_exact_stream(const SpiceyAcExact *x);
void spicey_ac_exact_dims(const SpiceyAcExact *x, int32_t *n_inst, int32_t *n_out, int32_t *n_cur, int32_t *n_v);
void spicey_ac_exact_info(const SpiceyAcExact *x, SpiceyInfo *info);
const char *spicey_ac_exact_error(const SpiceyAcExact *x);
void spicey_ac_exact_destroy(SpiceyAcExact *x);
