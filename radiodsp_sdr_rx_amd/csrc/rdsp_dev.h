/*
 * rdsp_dev.h -- the owners of HIP resources that the host objects (chain, engine, pre-processor) are made of: a device
 * allocation, a pinned host allocation, a stream, an event.  Each holds one handle, releases it in its destructor if it has
 * one, converts to the raw handle, and is neither copied nor moved: an object made of them is released by `delete`, once,
 * whatever set-up call failed half-way.  The destroy call of the object makes its device current first.
 */
#ifndef RDSP_DEV_H
#define RDSP_DEV_H

#include <hip/hip_runtime.h>

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

}  // namespace rdsp_dev
#endif
