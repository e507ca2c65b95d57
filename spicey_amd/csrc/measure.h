// measure.h — host-callable launcher of measure.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct SpiceyMeasDevReq;

// The two kernels of the measurement pass, enqueued on `st` behind a copy of `table` (HOST, validated and sorted:
// spicey_meas_plan of measure_exec.h) into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_measure(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                 const SpiceyMeasDevReq *table, int32_t n_req, double *d_meas, void *d_work, hipStream_t st);

// A request table (HOST, `bytes` long) into device memory by an asynchronous copy on `st`: the bytes are staged in a small
// ring of pinned buffers, so `table` may go away as soon as the call returns.  Shared with ac_measure.hip.
hipError_t spicey_upload_table_async(int device, void *d_dst, const void *table, size_t bytes, hipStream_t st);
