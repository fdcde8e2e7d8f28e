// What every C entry point of the libraries does the same way: report an error through the
// library's thread-local message, wrap a HIP call, own a device allocation for the call's duration.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mimo_engine.h"

namespace mimo {

// The library's one thread-local message: engine.hip defines it for libmimo_engine
// (mimo_last_error), probe.hip for libmimo_probe (mimo_probe_last_error).  Hidden, so that each
// library binds to its own however the two are loaded.
__attribute__((visibility("hidden"))) void set_error(const std::string& m);

inline int fail(int code, const std::string& m) {
  set_error(m);
  return code;
}

// (MIMO_EHIP is also probe.h's MIMO_PROBE_EHIP: probe.hip asserts it)
#define MIMO_HIP_TRY(expr)                                                                                    \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess) return mimo::fail(MIMO_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
  } while (0)

// An owned device allocation, freed at scope exit.
struct DBuf {
  void* p = nullptr;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
  template <typename T>
  T* as() { return reinterpret_cast<T*>(p); }
};

}  // namespace mimo
