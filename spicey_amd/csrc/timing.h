// timing.h — host-callable launcher of timing.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct SpiceyTimPlan;

// The timing pass, enqueued on `st`: a copy of the plan's head (HOST: edge and request tables; spicey_tim_judge of
// timing_exec.h) into the head of d_work, the base windows through spicey_launch_measure into the workspace's base rows
// (when the plan has any), then the two kernels of this pass.  The device must be current.  No synchronisation.
hipError_t spicey_launch_timing(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                const SpiceyTimPlan &plan, double *d_out, void *d_work, hipStream_t st);
