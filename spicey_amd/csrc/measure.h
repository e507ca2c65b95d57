// measure.h — host-callable launcher of measure.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct SpiceyMeasDevReq;

// The two kernels of the measurement pass, enqueued on `st` behind a copy of `table` (HOST, validated and sorted:
// spicey_meas_plan of measure_exec.h) into the head of d_work.  The device must be current.  No synchronisation.
hipError_t spicey_launch_measure(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                 const SpiceyMeasDevReq *table, int32_t n_req, double *d_meas, void *d_work, hipStream_t st);

// The grids of the reduction passes' launchers (measure.hip, ac_measure.hip, fourier.hip, timing.hip).  Stage 1: one
// workgroup per tile up to 2^20 (workgroups beyond this take several tiles each).  Stage 2: one thread per item in
// workgroups of `threads`; hipErrorInvalidValue for more workgroups than a launch takes.
inline unsigned spicey_meas_grid1(int64_t tiles) {
  const int64_t cap = (int64_t)1 << 20;
  return (unsigned)(tiles < cap ? tiles : cap);
}
inline hipError_t spicey_meas_grid2(int64_t total, int threads, unsigned *grid) {
  const int64_t g = (total + threads - 1) / threads;
  if (g > 0x7fffffffLL) return hipErrorInvalidValue;
  *grid = (unsigned)g;
  return hipSuccess;
}

// A request table (HOST, `bytes` long) into device memory by an asynchronous copy on `st`: the bytes are staged in a small
// ring of pinned buffers, so `table` may go away as soon as the call returns.  Shared with ac_measure.hip.
hipError_t spicey_upload_table_async(int device, void *d_dst, const void *table, size_t bytes, hipStream_t st);
// Before `st` is destroyed, with its work finished: the ring gives up the events it last recorded on `st` and takes the
// slots' buffers back.  (A waited-for event is looked up through the stream it was last recorded on; that stream must exist.)
void spicey_table_ring_release(hipStream_t st);
