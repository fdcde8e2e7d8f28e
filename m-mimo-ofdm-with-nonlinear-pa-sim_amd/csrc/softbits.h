// Max-log soft bits of a Gray-labelled square QAM axis and the reliability bins of the soft mode
// (include/mimo_engine.h mimo_engine_soft_points, mimo_qam_softbits): one device function shared by
// the trial kernel's soft instances (trial_kernel.h SOFT) and the stage kernel k_qam_softbits
// (stages.hip), so that the metric the fused kernel bins can be tested on crafted inputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mimo {

constexpr int kSoftBins = 256;  // MIMO_SOFT_BINS

// lambda_j(x) = (d0 - d1) (d0 + d1) / 4 for every Gray bit j = hb - 1 ... 0 of one axis, d_b the
// distance from x to the nearest level (odd integers -(L - 1) ... L - 1) whose Gray bit j is b;
// emit(j, lambda) is called MSB first.
//  - The nearest level's index i = clamp(floor(x / 2) + L / 2, 0, L - 1): x / 2 and floor are exact,
//    so no rounding decides it (floor((x + L) / 2) rounds x + L and can pick the neighbour, whose
//    distance differs in the last place).  At a midpoint either neighbour gives the same distances.
//  - Gray bit j of index i is bit j + 1 of s = i + 2^j: blocks of H = 2^(j+1) indices alternate
//    0, 1, 0 ... in s.  The nearest level of the other kind is the last index of the block below
//    or the first of the block above, whichever exists and is nearer; the nearest of i's own kind
//    is i.
//  - Every distance is |x - a| with an integer a: one IEEE operation.  No multiply feeds an add,
//    and contraction is switched off for the function all the same.
template <class Emit>
__device__ __forceinline__ void soft_axis(double x, int L, int hb, Emit&& emit) {
#pragma clang fp contract(off)
  const double half = (double)(L >> 1);
  const double fi = fmin(fmax(floor(x * 0.5), -half), half - 1.0);
  const int i = (int)fi + (L >> 1);
  const double d_same = fabs(x - (double)(2 * i - (L - 1)));
  for (int j = hb - 1; j >= 0; --j) {
    const int q = 1 << j, H = q << 1;
    const int s = i + q;
    const int base = s & ~(H - 1);
    const int i_lo = base - 1 - q, i_hi = base + H - q;
    const double d_lo = i_lo >= 0 ? fabs(x - (double)(2 * i_lo - (L - 1))) : __builtin_huge_val();
    const double d_hi = i_hi < L ? fabs(x - (double)(2 * i_hi - (L - 1))) : __builtin_huge_val();
    const double d_opp = fmin(d_lo, d_hi);
    const bool one = (s >> (j + 1)) & 1;
    const double d0 = one ? d_opp : d_same, d1 = one ? d_same : d_opp;
    emit(j, (d0 - d1) * (d0 + d1) * 0.25);
  }
}

// bin of the reliability rho = +-lambda of a transmitted bit: clamp(floor(rho scale), -128, 127) + 128,
// the clamp in double before the conversion (scale = 128 / rho_max, formed on the host)
__device__ __forceinline__ int soft_bin(double lambda, bool bit, double scale) {
#pragma clang fp contract(off)
  const double rho = bit ? lambda : -lambda;
  const double f = floor(rho * scale);
  return (int)fmin(fmax(f, -128.0), 127.0) + 128;
}

// channel value of the coded mode from the same reliability: c = 2 clamp(floor(rho scale), -32, 31) + 1,
// the clamp in double before the conversion (scale = 32 / rho_max, formed on the host): an odd
// integer in [-63, 63], c < 0 a hard-decision error.  Its 64 bins' edges are soft_bin's at the same
// rho_max.
__device__ __forceinline__ int coded_value(double lambda, bool bit, double scale) {
#pragma clang fp contract(off)
  const double rho = bit ? lambda : -lambda;
  const double f = floor(rho * scale);
  return 2 * (int)fmin(fmax(f, -32.0), 31.0) + 1;
}

}  // namespace mimo
