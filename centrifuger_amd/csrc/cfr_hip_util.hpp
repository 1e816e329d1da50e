// cfr_hip_util.hpp — the HIP plumbing the device translation units share: the error check, the device scope and one owner for every
// kind of runtime object.  Internal: not installed, not reachable from include/cfr_hip.h.
//
// Everything is local to the including file (unnamed namespace): a file that wants its messages to begin with a name of its own
// defines CFR_HIP_PREFIX before the include ("index build: " in cfr_build_sa.hip), and the owners then report with that prefix too.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "cfr_device.hpp"      // HipError

#ifndef CFR_HIP_PREFIX
#define CFR_HIP_PREFIX ""
#endif

namespace cfr {
namespace {

inline void hip_check(hipError_t e, const char *what, const char *prefix = "") {
  if (e != hipSuccess) throw HipError{std::string(prefix) + what + ": " + hipGetErrorString(e), (int)e};
}
#define HIP_CHECK(x) hip_check((x), #x, CFR_HIP_PREFIX)

inline bool device_exists(int device) {
  int count = 0;
  return hipGetDeviceCount(&count) == hipSuccess && device >= 0 && device < count;
}

// the calling thread's current device is put back when a call returns: the classifier's workers drive other GPUs on the same threads
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; HIP_CHECK(hipSetDevice(d)); }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline unsigned grid_for(size_t n, int block = 256) { return (unsigned)((n + block - 1) / block); }

// Owners: move-only, empty by default, released by the destructor - so whatever a constructor or a call has allocated when a later
// step throws goes back to the device without a list of pointers kept by hand.  alloc() lets go of the old memory first.
template <class T, class Mem> class OwnedBuf {
 public:
  OwnedBuf() = default;
  explicit OwnedBuf(size_t n) { alloc(n); }
  OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept { std::swap(p_, o.p_); return *this; }
  ~OwnedBuf() { reset(); }
  void alloc(size_t n) { reset(); p_ = (T *)Mem::alloc(std::max<size_t>(n * sizeof(T), 16)); }
  void reset() { if (p_) Mem::free(p_); p_ = nullptr; }
  void adopt(T *p) { reset(); p_ = p; }                // memory of the same kind that another owner has released
  T *release() { T *p = p_; p_ = nullptr; return p; }
  T *get() const { return p_; }
  operator T *() const { return p_; }

 private:
  T *p_ = nullptr;
};
struct DeviceMem {
  static void *alloc(size_t bytes) { void *p = nullptr; HIP_CHECK(hipMalloc(&p, bytes)); return p; }
  static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
  static void *alloc(size_t bytes) { void *p = nullptr; HIP_CHECK(hipHostMalloc(&p, bytes, hipHostMallocDefault)); return p; }
  static void free(void *p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = OwnedBuf<T, DeviceMem>;        // hipMalloc, at least 16 bytes
template <class T> using PinnedBuf = OwnedBuf<T, PinnedMem>;     // hipHostMalloc(hipHostMallocDefault)

// a non-blocking stream / an event with default flags (its times are read); made by create(), not by the constructor, because the
// device they belong to is chosen in the owner's constructor body
class Stream {
 public:
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  void create() { HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};
class Event {
 public:
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  void create() { HIP_CHECK(hipEventCreate(&e_)); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace
}  // namespace cfr
