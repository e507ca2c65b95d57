// ac_measure.h — host-callable launcher of ac_measure.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct SpiceyAcMeasDevReq;

// The kernel of the AC measurement pass, enqueued on `st` behind a copy of `table` (HOST, validated and sorted:
// spicey_acm_plan of ac_measure_exec.h) into d_work.  d_v [n_inst][n_freq][n_v][2], d_i likewise or null, d_meas
// [n_inst][n_req][8].  The device must be current.  No synchronisation.
hipError_t spicey_launch_ac_measure(int device, int32_t n_inst, int64_t n_freq, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                    const SpiceyAcMeasDevReq *table, int32_t n_req, double *d_meas, void *d_work, hipStream_t st);
