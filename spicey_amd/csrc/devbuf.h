// devbuf.h — owned device memory of the host runtime: DevBuf<T> (hipFree in its destructor), the one upload helper and
// the HIP-call check of the C-ABI entry points.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <string>

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
