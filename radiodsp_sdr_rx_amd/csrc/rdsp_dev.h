/*
 * rdsp_dev.h -- the owners of HIP resources that the host objects (chain, engine, pre-processor) are made of: a device
 * allocation, a pinned host allocation, a stream, an event.  Each holds one handle, releases it in its destructor if it has
 * one, converts to the raw handle, and is neither copied nor moved: an object made of them is released by `delete`, once,
 * whatever set-up call failed half-way.  The destroy call of the object makes its device current first.
 */
#ifndef RDSP_DEV_H
#define RDSP_DEV_H

#include <hip/hip_runtime.h>

#include "rdsp_host.h"

namespace rdsp_dev {

template <typename T>
struct DevBuf {
  T *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  hipError_t alloc(size_t n) { release(); return hipMalloc((void **)&p, n * sizeof(T)); }
  void release() { if (p) (void)hipFree(p); p = nullptr; }
  operator T *() const { return p; }
};
/* n zeroed elements (hipMemset: the caller's device is current, nothing of the buffer is queued yet) */
template <typename T> static inline hipError_t alloc_zero(DevBuf<T> &b, size_t n) {
  const hipError_t e = b.alloc(n);
  return e != hipSuccess ? e : hipMemset(b.p, 0, n * sizeof(T));
}

template <typename T>
struct PinnedBuf { /* hipHostMalloc */
  T *p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t n) { return hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault); }
  operator T *() const { return p; }
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream &) = delete; Stream &operator=(const Stream &) = delete;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
  operator hipStream_t() const { return s; }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event &) = delete; Event &operator=(const Event &) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};

/* a HIP call returned e != hipSuccess */
static inline int hip_fail(const char *expr, hipError_t e, const char *file, int line) {
  rdsp_set_error("%s failed: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
  return RDSP_ERR_HIP;
}

/* in front of every create that has no wording of its own for it: RDSP_OK, or the refusal on a machine without a device */
static inline int need_device() {
  if (rdsp_device_count() > 0) return RDSP_OK;
  rdsp_set_error("no HIP device: the rdsp product path has no CPU fallback");
  return RDSP_ERR_NO_DEVICE;
}

}  // namespace rdsp_dev

/* the try macros of every host file: a failed HIP call sets the error text and returns RDSP_ERR_HIP, a failed rdsp call
 * returns its code */
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return rdsp_dev::hip_fail(#expr, e_, __FILE__, __LINE__);           \
  } while (0)
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_ != RDSP_OK) return rc_; } while (0)
#endif
