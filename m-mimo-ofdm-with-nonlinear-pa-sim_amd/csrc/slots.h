// Which in-band sub-carriers ("slots") a thread of the trial kernel's team owns, and where they sit
// among its FFT registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "real.h"

namespace mimo {

// ---------------------------------------------------------------- slot geometry
// ALIGNED: S % (4T) == 0 and S < F.  Slot s < HALF is the positive band (bin
// n = t + T s, k = n + S/2 - 1; thread 0 slot 0 is bin S/2 instead of DC); slot s >= HALF
// is the negative band (bin F - S/2 + t + T (s - HALF), k = t + T (s - HALF)).
// Generic: slot s = register s, valid iff its bin is in band.
template <int F, int T, int NSLOT, bool ALIGNED>
struct Slots {
  static constexpr int P = F / T;
  static constexpr int HALF = NSLOT / 2;
  static constexpr int m_of(int s) { return ALIGNED ? (s < HALF ? s : P - NSLOT + s) : s; }
  // Registers the scatter leaves zero in every thread: the out-of-band middle
  // (HALF + 1 .. P - HALF - 1; register HALF holds thread 0's bin S/2).  Generic: none.
  static constexpr uint32_t zero_mask() {
    uint32_t m = 0;
    if (ALIGNED)
      for (int r = HALF + 1; r < P - HALF; ++r) m |= 1u << r;
    return m;
  }

  static __device__ __forceinline__ int k_of(int s, int t, int S, bool& valid) {
    if constexpr (ALIGNED) {
      valid = true;
      if (s < HALF) {
        const int n = (s == 0 && t == 0) ? (S >> 1) : t + T * s;
        return n + (S >> 1) - 1;
      }
      return t + T * (s - HALF);
    } else {
      const int n = t + T * s;
      const int lo = F - (S >> 1);
      valid = (n >= 1 && n <= (S >> 1)) || n >= lo;
      return !valid ? 0 : (n >= lo ? n - lo : n + (S >> 1) - 1);  // 0 keeps table reads in bounds
    }
  }

  template <class C>
  static __device__ __forceinline__ void scatter(C (&d)[P], const C (&x)[NSLOT], bool t0) {
    using R = real_of<C>;
#pragma unroll
    for (int m = 0; m < P; ++m) d[m] = czero<R>();
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      if constexpr (ALIGNED) {
        if (s == 0) {
          // thread 0's slot 0 is bin S/2 (register HALF), the others' bin t (register 0):
          // two multiplies by 0 / 1 per component instead of four 32-bit selects
          const R m1 = t0 ? R(1) : R(0), m0 = R(1) - m1;
          d[0] = cscale(x[0], m0);
          d[HALF] = cscale(x[0], m1);
          continue;
        }
      }
      d[m_of(s)] = x[s];
    }
  }

  template <class C>
  static __device__ __forceinline__ C gather(const C (&d)[P], int s, bool t0) {
    if constexpr (ALIGNED) {
      if (s == 0) return t0 ? d[HALF] : d[0];
    }
    return d[m_of(s)];
  }
};

}  // namespace mimo
