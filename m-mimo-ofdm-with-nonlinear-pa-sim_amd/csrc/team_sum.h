// Wave and team reductions of the trial kernel, and the opaque copy that keeps derived values out of
// its antenna loop's preheader.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mimo {

// ---------------------------------------------------------------- small helpers
// Opaque copy: stops LICM from hoisting thread-invariant derived values (slot->k maps,
// Philox round-0 products, QAM points, table loads) out of the antenna loop, which
// would keep dozens of VGPRs live across it and spill.  Re-deriving them is cheap.
template <typename V>
__device__ __forceinline__ V opaque(V v) {
  asm volatile("" : "+v"(v));
  return v;
}
template <typename R>
__device__ __forceinline__ R wave_sum(R v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Wave sum delivered in lane 63 only (other lanes hold partial sums): DPP adds on the
// VALU instead of the six dependent ds_bpermute round trips of __shfl_xor.  Per row of
// 16 lanes: pair / quad swaps and the half-row / row mirrors give every lane its row sum;
// row_bcast:15 then row_bcast:31 fold rows 0-2 into row 3.  (fp64: both halves moved.)
// mov_dpp leaves the lanes of disabled rows undefined (no zero-initialised "old" operand,
// one v_mov fewer per step): after the row_bcast:15 step rows 0 and 2 hold garbage, which
// no later step reads (row_bcast:31 reads lane 31, row 1) and lane 63 never sees.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_add(float v) {
  const int s = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false);
  return v + __builtin_bit_cast(float, s);
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_add(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, ROW_MASK, 0xF, false);
  return v + __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
template <typename R>
__device__ __forceinline__ R wave_sum_lane63(R v) {
  v = dpp_add<0xB1>(v);        // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);        // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);       // row_half_mirror
  v = dpp_add<0x140>(v);       // row_mirror
  v = dpp_add<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
  return v;
}

// Team-wide sum; every thread gets the result.  Two barriers.
template <int T, typename R>
__device__ __forceinline__ R team_sum(R v, R* red) {
  if constexpr (T == 64) {
    return wave_sum(v);
  } else {
    v = wave_sum_lane63(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
    __syncthreads();
    R s = R(0);
#pragma unroll
    for (int i = 0; i < T / 64; ++i) s += red[i];
    return s;
  }
}

}  // namespace mimo
