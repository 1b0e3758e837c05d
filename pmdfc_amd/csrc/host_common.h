// host_common.h -- what the host files of the engine library share: the
// error text behind pmdfc_last_error, the return-on-error macro, and the
// scoped device guard and temporaries.  Host only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/pmdfc_cceh.h"

namespace pmdfc {

// The calling thread's error text (pmdfc_last_error): one string per thread,
// defined in cceh_engine.hip.  A caller reads it on the thread that failed.
std::string& last_error();

inline int fail(int code, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(buf, sizeof buf, "%s", what);
  last_error() = buf;
  return code;
}

#define HIPCHK(x)                                   \
  do {                                              \
    hipError_t e_ = (x);                            \
    if (e_ != hipSuccess) return fail(PMDFC_ERR_HIP, #x, e_); \
  } while (0)

inline uint32_t ceil_log2(uint64_t v) {
  uint32_t b = 0;
  while ((1ULL << b) < v) ++b;
  return b;
}

struct DevGuard {
  int prev = -1;
  explicit DevGuard(int d) {
    (void)hipGetDevice(&prev);
    if (prev != d) (void)hipSetDevice(d);
  }
  ~DevGuard() {
    int cur;
    (void)hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
};

struct DevTmp {  // a device allocation that lives for one synchronous call
  void* p = nullptr;
  ~DevTmp() {
    if (p) (void)hipFree(p);
  }
};

// Its stream-ordered twin: a hipMallocAsync block bound to its stream, freed
// on it at scope end (after every launch enqueued before that reads it).
// Declare it after the DevGuard that must still hold when it is freed.
struct StreamTmp {
  void* p = nullptr;
  hipStream_t s = nullptr;
  hipError_t alloc(size_t bytes, hipStream_t stream) {
    s = stream;
    return hipMallocAsync(&p, bytes, s);
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  ~StreamTmp() {
    if (p) (void)hipFreeAsync(p, s);
  }
};

}  // namespace pmdfc
