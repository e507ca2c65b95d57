// fourier.h — host-callable launcher of fourier.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct SpiceyFourPlan;

// The two kernels of the harmonics pass, enqueued on `st` behind a copy of the plan's head (HOST: request table, bases and
// the twiddles built for `dt`; spicey_four_judge of fourier_exec.h) into the head of d_work.  The device must be current.
// No synchronisation.
hipError_t spicey_launch_fourier(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                 const SpiceyFourPlan &plan, double *d_out, int32_t out_stride, void *d_work, hipStream_t st);
