// devbuf.h — what the host runtime's sources share: DevBuf<T> (owned device memory, hipFree in its destructor), the one
// upload helper, the HIP-call check of the C-ABI entry points, the device open, the numbering of the reduction passes,
// StreamTimers (a stream, the event pair of its kernel and one pair per reduction pass), the dynamic-LDS rule of the
// transient and AC launchers and the refusals of a measurement call (spicey_judge_measure).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/spicey_hip.h"

// A HIP call in an entry point: on failure `h->err` = the call's text and the runtime's message, return SPICEY_ERR_HIP.
#define HIPCHK(h, call)                                                                                                   \
  do {                                                                                                                    \
    hipError_t e__ = (call);                                                                                              \
    if (e__ != hipSuccess) { (h)->err = std::string(#call) + ": " + hipGetErrorString(e__); return SPICEY_ERR_HIP; }      \
  } while (0)

// A device allocation of `T`s, move-only; null until alloc() succeeds.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t count) { reset(); return hipMalloc((void **)&p_, count * sizeof(T)); }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
};

// max(count, 1) elements (a kernel argument is never null) holding `src`, or zeros when there is no source data
template <class T>
hipError_t dev_upload(DevBuf<T> &dst, size_t count, const T *src = nullptr) {
  const hipError_t e = dst.alloc(count ? count : 1);
  if (e != hipSuccess) return e;
  return count && src ? hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(dst, 0, (count ? count : 1) * sizeof(T));
}

// Ordinal check, selection and CU count of `device` (spicey_plan calls it after the descriptor checks: PlanDevice::open).
inline int32_t spicey_open_device(int device, int *ncu, std::string &err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { err = "no HIP device: libspicey_hip has no CPU path"; return SPICEY_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { err = "device ordinal out of range"; return SPICEY_ERR_BAD_DESC; }
  if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return SPICEY_ERR_HIP; }
  (void)hipDeviceGetAttribute(ncu, hipDeviceAttributeMultiprocessorCount, device);
  return SPICEY_OK;
}

// The reduction passes behind a transient run, in the order they run (reduced_abi.cpp, run_reduced): the index of a pass's
// event pair in StreamTimers and of its time in SpiceyHandle::last_pass_ms.
enum SpiceyPass { PASS_MEASURE = 0, PASS_FOURIER = 1, PASS_TIMING = 2, PASS_SPECTRUM = 3, PASS_POWER = 4, PASS_VALUES = 5, N_PASS = 6 };

void spicey_table_ring_release(hipStream_t st);  // measure.hip: the staging ring of the request tables

// A handle's stream and its timing events: ev0 / ev1 bracket the kernel of a run, pass_ev[p] the reduction pass p of a
// *_run_measure* (created on first use; an AC handle has the measurement pass only).  Destroys what it created.  A handle
// declares it AFTER its DevBufs: members go in reverse order, so events and stream are destroyed before the device memory
// is freed.
struct StreamTimers {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t pass_ev[N_PASS][2] = {};
  StreamTimers() = default;
  StreamTimers(const StreamTimers &) = delete;
  ~StreamTimers() {
    for (hipEvent_t e : {ev0, ev1})
      if (e) (void)hipEventDestroy(e);
    for (auto &pair : pass_ev)
      for (hipEvent_t e : pair)
        if (e) (void)hipEventDestroy(e);
    if (stream) {
      // (the ring of request tables holds events recorded on this stream: they go while the stream still exists)
      (void)hipStreamSynchronize(stream);
      spicey_table_ring_release(stream);
      (void)hipStreamDestroy(stream);
    }
  }
  template <class H>
  int32_t create(H *h) {
    if (hipStreamCreate(&stream) == hipSuccess && hipEventCreate(&ev0) == hipSuccess && hipEventCreate(&ev1) == hipSuccess) return SPICEY_OK;
    h->err = "stream/event creation failed";
    return SPICEY_ERR_HIP;
  }
  hipError_t want_pass_events(int pass) {
    for (hipEvent_t &e : pass_ev[pass]) {
      const hipError_t err = e ? hipSuccess : hipEventCreate(&e);
      if (err != hipSuccess) return err;
    }
    return hipSuccess;
  }
  // elapsed milliseconds of a finished pair into *ms (left alone when the runtime cannot tell)
  static void elapsed(hipEvent_t a, hipEvent_t b, double *ms) {
    float f = 0.f;
    if (hipEventElapsedTime(&f, a, b) == hipSuccess) *ms = f;
  }
};

// Before the launch of `kernel` with `lds` bytes of dynamic LDS: above 48 KiB the runtime wants the limit raised first.
template <class K>
hipError_t spicey_allow_dyn_lds(K kernel, size_t lds) {
  if (lds <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// Every refusal of a measurement call, judged before the device is touched (a refusal launches nothing): counts, buffers,
// the request list (plan = spicey_meas_plan / spicey_acm_plan -> the kernels' sorted table), the workspace size.  kind =
// "measure" / "ac measure", the prefix of the texts.
template <class Req, class DevReq>
int32_t spicey_judge_measure(const char *kind, bool (*plan)(const Req *, int32_t, int64_t, int32_t, int32_t, bool, std::vector<DevReq> &, std::string &),
                             int64_t (*ws_bytes)(int32_t, int64_t, int32_t), int32_t n_inst, int64_t n_points, bool have_v, int32_t n_v, bool have_i, int32_t n_i,
                             const Req *reqs, int32_t n_req, bool have_out, int64_t work_bytes, std::vector<DevReq> &table, std::string &err) {
  if (n_inst <= 0 || n_v < 0 || n_i < 0 || !have_out) { err = std::string(kind) + ": bad arguments (n_inst >= 1, result and workspace buffers)"; return SPICEY_ERR_BAD_DESC; }
  if (!plan(reqs, n_req, n_points, have_v ? n_v : 0, n_i, have_i, table, err)) return SPICEY_ERR_BAD_DESC;
  const int64_t need = ws_bytes(n_inst, n_points, n_req);
  if (work_bytes < need) {
    std::string fn = std::string("spicey_") + kind + "_workspace_bytes";
    std::replace(fn.begin(), fn.end(), ' ', '_');
    char buf[192];
    snprintf(buf, sizeof(buf), "%s: workspace of %lld bytes is too small, %lld needed (%s)", kind, (long long)work_bytes, (long long)need, fn.c_str());
    err = buf;
    return SPICEY_ERR_BAD_DESC;
  }
  return SPICEY_OK;
}
