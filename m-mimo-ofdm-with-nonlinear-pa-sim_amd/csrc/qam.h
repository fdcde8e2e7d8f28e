// Square Gray-coded QAM on the device: the hard slicer and the label -> point maps, shared by the
// trial kernel and the fine-seam stage kernels (stages.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "real.h"

namespace mimo {

// Per-axis hard slicer == argmin |z - C| over the Gray-ordered constellation with the
// reference's first-index (lowest label) tie-break (modulation.py:75-76,138-146).
__device__ __forceinline__ uint32_t gray(uint32_t i) { return i ^ (i >> 1); }
__device__ __forceinline__ uint32_t gray_inv(uint32_t g) {
  g ^= g >> 1;
  g ^= g >> 2;
  g ^= g >> 4;
  g ^= g >> 8;
  return g;
}
template <typename R>
__device__ __forceinline__ uint32_t slice_axis(R x, int L) {
  const R q = (x + (R)L) * R(0.5);
  const R fi = floor_r(q);
  int i = (int)fi;
  if (q == fi && i > 0 && i < L) {  // exact midpoint between levels i-1 and i
    i = gray((uint32_t)(i - 1)) < gray((uint32_t)i) ? i - 1 : i;
  }
  i = i < 0 ? 0 : (i > L - 1 ? L - 1 : i);
  return gray((uint32_t)i);
}
template <class C>
__device__ __forceinline__ uint32_t slice(C z, int L, int hb) {
  return (slice_axis(z.x, L) << hb) | slice_axis(z.y, L);
}
template <typename R>
__device__ __forceinline__ cx<R> qam_point(uint32_t label, int L, int hb) {
  const uint32_t ii = gray_inv(label >> hb), iq = gray_inv(label & ((1u << hb) - 1u));
  return mkc((R)(2 * (int)ii - (L - 1)), (R)(2 * (int)iq - (L - 1)));
}
// The same point as two int16 lattice levels in one word (I high, Q low): the register
// diet keeps these per slot and rebuilds the point per antenna in 2 shifts + 2 converts
// instead of the two inverse Gray codes (~20 integer ops).
__device__ __forceinline__ uint32_t qam_levels(uint32_t label, int L, int hb) {
  const int ii = 2 * (int)gray_inv(label >> hb) - (L - 1), iq = 2 * (int)gray_inv(label & ((1u << hb) - 1u)) - (L - 1);
  return ((uint32_t)ii << 16) | ((uint32_t)iq & 0xFFFFu);
}
// Two slots per word for the register diet: int8 lattice levels (|level| <= L - 1 <= 63 for
// M <= 4096), slot 2 i + h in bits 16 h .. 16 h + 15 of word i (I high byte): half the VGPRs
// of one word per slot, and the same 2 extracts + 2 converts (v_bfe_i32) to rebuild.
__device__ __forceinline__ uint32_t qam_levels8(uint32_t label, int L, int hb) {
  const int ii = 2 * (int)gray_inv(label >> hb) - (L - 1), iq = 2 * (int)gray_inv(label & ((1u << hb) - 1u)) - (L - 1);
  return (((uint32_t)ii & 0xFFu) << 8) | ((uint32_t)iq & 0xFFu);
}
template <typename R, int H>
__device__ __forceinline__ cx<R> levels_point8(uint32_t w) {
  // sign-extending extracts of bits 16 H + 8 .. + 15 (I) and 16 H .. + 7 (Q)
  return mkc((R)((int)(w << (16 - 16 * H)) >> 24), (R)((int)(w << (24 - 16 * H)) >> 24));
}
template <typename R>
__device__ __forceinline__ cx<R> levels_point(uint32_t v) {
  return mkc((R)((int)v >> 16), (R)(int)(int16_t)(v & 0xFFFFu));
}

}  // namespace mimo
