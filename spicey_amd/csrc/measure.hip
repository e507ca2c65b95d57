// measure.hip — device-side waveform measurements (spicey_measure_device): kernels and launcher.
//
// A reduction pass of its own over the step-major buffers [inst][step][col] a transient kernel wrote; measure_exec.h holds
// the arithmetic and the mapping, shared with the CPU harness of tests/measure_host.  Two kernels, no atomics, no waiting
// on other workgroups:
//   stage 1  one thread per (request, chunk of SPICEY_MEAS_CHUNK steps): the lanes of a wave take neighbouring requests —
//            the table is sorted by column, so a wave instruction reads neighbouring addresses of one row and the
//            all-columns case streams whole rows — and with fewer requests than lanes the rest of the workgroup spreads
//            over chunks.  Each thread walks its chunk in step order and leaves 8 doubles in the workspace.
//   stage 2  one thread per (instance, request) adds the request's chunk partials in ascending chunk order and writes the
//            row of `meas` the caller's list names.
// Bit identity with the CPU harness needs every product and sum rounded on its own: no FMA contraction in this
// translation unit (as exact.hip).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "measure.h"
#include "measure_exec.h"

namespace {

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_measure_stage1(int32_t n_inst, int64_t n_points, double dt, const double *__restrict__ a_v, int32_t n_v,
                                                                             const double *__restrict__ a_i, int32_t n_i,
                                                                             const SpiceyMeasDevReq *__restrict__ table, int32_t n_req,
                                                                             double *__restrict__ partials) {
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_req, SPICEY_MEAS_THREADS);
  for (int64_t tile = blockIdx.x; tile < g.tiles; tile += gridDim.x)
    spicey_meas_stage1(g, tile, (int32_t)threadIdx.x, table, n_req, n_points, dt, a_v, n_v, a_i, n_i, partials);
}

__global__ void __launch_bounds__(SPICEY_MEAS_THREADS) spicey_measure_stage2(int64_t total, const SpiceyMeasDevReq *__restrict__ table, int32_t n_req,
                                                                             int64_t max_chunks, const double *__restrict__ partials,
                                                                             double *__restrict__ meas) {
  const int64_t idx = (int64_t)blockIdx.x * SPICEY_MEAS_THREADS + threadIdx.x;
  if (idx < total) spicey_meas_stage2(idx, table, n_req, max_chunks, partials, meas);
}

// The request table goes to the device by an asynchronous copy, so its host copy must outlive the call: a small ring of
// pinned buffers, each reused only after the copy that last read it has finished (an event per slot; the wait happens only
// when SLOTS launches are in flight).  An event is not touched again once the stream it was last recorded on is gone:
// the runtime keeps that stream's address in the event and looks at it when the event is waited for, so a handle that
// destroys its stream releases its slots first (spicey_table_ring_release).
struct TableRing {
  static const int SLOTS = 8;
  std::mutex mu;
  struct Slot { void *p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; int device = -1; hipStream_t stream = nullptr; } slot[SLOTS];
  int next = 0;
};
TableRing &table_ring() {
  static TableRing *r = new TableRing();  // (never freed: the runtime may be gone when statics are destroyed)
  return *r;
}

}  // namespace

hipError_t spicey_upload_table_async(int device, void *d_dst, const void *table, size_t bytes, hipStream_t st) {
  hipError_t e;
  TableRing &ring = table_ring();
  std::lock_guard<std::mutex> lk(ring.mu);
  TableRing::Slot &s = ring.slot[ring.next];
  ring.next = (ring.next + 1) % TableRing::SLOTS;
  if (s.used) {
    if ((e = hipEventSynchronize(s.ev)) != hipSuccess) return e;
    s.used = false;
  }
  if (s.ev && s.device != device) {  // (an event belongs to the device it was created on)
    (void)hipEventDestroy(s.ev);
    s.ev = nullptr;
  }
  if (!s.ev) {
    if ((e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming)) != hipSuccess) return e;
    s.device = device;
  }
  if (s.cap < bytes) {
    if (s.p) (void)hipHostFree(s.p);
    s.p = nullptr;
    s.cap = 0;
    if ((e = hipHostMalloc(&s.p, bytes, hipHostMallocDefault)) != hipSuccess) return e;
    s.cap = bytes;
  }
  memcpy(s.p, table, bytes);
  if ((e = hipMemcpyAsync(d_dst, s.p, bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipEventRecord(s.ev, st)) != hipSuccess) return e;
  s.used = true;
  s.stream = st;
  return hipSuccess;
}

void spicey_table_ring_release(hipStream_t st) {
  TableRing &ring = table_ring();
  std::lock_guard<std::mutex> lk(ring.mu);
  for (TableRing::Slot &s : ring.slot)
    if (s.ev && s.stream == st) {
      (void)hipEventDestroy(s.ev);
      s.ev = nullptr;
      s.used = false;
      s.stream = nullptr;
    }
}

hipError_t spicey_launch_measure(int device, int32_t n_inst, int64_t n_points, double dt, const double *d_v, int32_t n_v, const double *d_i, int32_t n_i,
                                 const SpiceyMeasDevReq *table, int32_t n_req, double *d_meas, void *d_work, hipStream_t st) {
  hipError_t e;
  if ((e = spicey_upload_table_async(device, d_work, table, (size_t)n_req * sizeof(SpiceyMeasDevReq), st)) != hipSuccess) return e;
  const SpiceyMeasDevReq *d_table = (const SpiceyMeasDevReq *)d_work;
  double *partials = (double *)((char *)d_work + spicey_meas_head_bytes(n_req));
  const SpiceyMeasGeom g = spicey_meas_geom(n_inst, n_points, n_req, SPICEY_MEAS_THREADS);
  hipLaunchKernelGGL(spicey_measure_stage1, dim3(spicey_meas_grid1(g.tiles)), dim3(SPICEY_MEAS_THREADS), 0, st, n_inst, n_points, dt, d_v, n_v, d_i, n_i, d_table, n_req, partials);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int64_t total = (int64_t)n_inst * n_req;
  unsigned grid2 = 0;
  if ((e = spicey_meas_grid2(total, SPICEY_MEAS_THREADS, &grid2)) != hipSuccess) return e;
  hipLaunchKernelGGL(spicey_measure_stage2, dim3(grid2), dim3(SPICEY_MEAS_THREADS), 0, st, total, d_table, n_req, g.max_chunks, (const double *)partials, d_meas);
  return hipGetLastError();
}
