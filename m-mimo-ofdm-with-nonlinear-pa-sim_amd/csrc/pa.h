// The power amplifier of the trial kernel's transmit chain (pa_block, on a thread's time-domain
// samples) and the Bussgang gain's exact formula.
#pragma once
#include <hip/hip_runtime.h>

#include "real.h"
#include "trial_params.h"

namespace mimo {

// Bussgang gain, modulation.py:178-189, from gamma^2.
__device__ __forceinline__ float alpha_of_gamma2(float g2) {
  const float g = __builtin_sqrtf(g2);
  return 1.0f - __expf(-g2) + 0.88622692545275801f * g * erfcf(g);
}
__device__ __forceinline__ double alpha_of_gamma2(double g2) {
  const double g = __builtin_sqrt(g2);
  return 1.0 - exp(-g2) + 0.88622692545275801 * g * erfc(g);
}

// PA on one time-domain sample (distortion.py:9-19, 102-113, 202-211).
// Soft limiter: min(1, sqrt(sat) rsq(pw)) -- the reference's branch |x|^2 > sat, then
// x sqrt(sat / |x|^2), up to rounding at |x|^2 = sat (fp64: -0.4 % against the branch).
// fp64 gains stay within 4 units of 2^-52 of the exact formulas (tests/test_gpu_probe_math.py):
// the soft limiter's rsq by one third-order step (real.h rsq_h1), the general-hardness Rapp
// gain with both powers on a base in [1, 2] (below).
template <class C, typename R = real_of<C>>
__device__ __forceinline__ C pa_apply(int kind, C x, R sat, R sqrt_sat, R inv_sat, R rapp_p, R toi) {
  const R pw = fmar(x.x, x.x, x.y * x.y);
  R sc = R(1);
  if (kind == PA_SOFTLIM) {
    if constexpr (sizeof(R) == 4) sc = minr(1.0f, sqrt_sat * rsq_r(pw));
    else sc = fmin(R(1), sqrt_sat * rsq_h1(pw));  // rsq(0) = inf -> NaN -> fmin picks 1
  } else if (kind == PA_RAPP) {
    // 1 / (1 + (pw/sat)^p)^(1/(2p))
    const R u = pw * inv_sat;
    if constexpr (sizeof(R) == 8) {
      // fp64 (cold path): exp2(-(1 / 2p) log2(1 + exp2(p log2 u))) loses ~0.5 |log2 u| ulp to
      // the rounding of p log2 u and of 1 / 2p (8.8 and 11.6 units of 2^-52 at p = 5 and 2.5,
      // u up to 10^6).  Above u = 1 the gain is u^(-1/2) (1 + u^-p)^(-1/2p) instead, so the
      // rounded exponent -1 / 2p only ever meets a base in [1, 2].
      const bool big = u > R(1);
      const R v = u > R(0) ? pow(u, big ? -rapp_p : rapp_p) : R(0);
      const R g = pow(R(1) + v, -(R(0.5) / rapp_p));
      sc = big ? g / __builtin_sqrt(u) : g;
    } else {
      const R up = u > R(0) ? exp2_r(rapp_p * log2_r(u)) : R(0);
      sc = exp2_r(-(R(0.5) / rapp_p) * log2_r(R(1) + up));
    }
  } else if (kind == PA_TOI) {
    sc = R(1) - toi * pw;
  }
  return mkc(x.x * sc, x.y * sc);
}

// Cold path out of line: the general-hardness Rapp gain (library pow).  Inlined,
// its f64 constants were hoisted into the loop preheader and spilled to scratch once per
// trial (~90 KB of writes per trial at config 2, profiles/r03/pmc); out of line they stay
// in the call.  Measured with the exact-alpha fallback (now alpha_fit.h's segment table,
// which has no constants to hoist) outlined as well: config 2 -2.5 %, CSI -2.7 %, LoS
// -2.3 %, two-path -3.0 %, F 8192 -0.4 %; F 4096 +1.6 % (profiles/r03/ab_s/).
template <class C, typename R = real_of<C>>
__device__ __attribute__((noinline)) C pa_rapp_general(C x, R inv_sat, R rapp_p) {
  return pa_apply(PA_RAPP, x, R(0), R(0), inv_sat, rapp_p, R(0));
}

// y^(-1/N) for y >= 1 (the Rapp gain at integer hardness, N = 2p).  fp32: hardware
// log / exp.  fp64: the fp32 hardware value z as the seed (~2^-22) and one third-order
// step z (1 - e)^(-1/N) ~ z (1 + e/N + (N+1) e^2 / (2 N^2)), e = 1 - y z^N (error
// ~2^-60, below the fp64 rounding): 7 f64 ops + 2 fp32 transcendentals instead of the
// library log2 + exp2 (~60 instructions).
template <int N>
__device__ __forceinline__ float rpow_neg_inv(float y) {
  return __builtin_amdgcn_exp2f((-1.0f / N) * __builtin_amdgcn_logf(y));
}
template <int N>
__device__ __forceinline__ double rpow_neg_inv(double y) {
  static_assert(N == 4 || N == 6, "integer Rapp hardness 2 or 3");
  const double z = (double)rpow_neg_inv<N>((float)y);
  const double z2 = z * z;
  const double zn = N == 4 ? z2 * z2 : z2 * z2 * z2;
  const double e = fma(-y, zn, 1.0);
  const double c = e * fma(e, (N + 1.0) / (2.0 * N * N), 1.0 / N);
  return fma(z, c, z);
}

// Rapp with an integer hardness: (pw/sat)^p by multiplication (config 5 uses p = 3), then
// (1 + (pw/sat)^p)^(-1/(2p)) by rpow_neg_inv.
template <int IP, int P, class C, typename R = real_of<C>>
__device__ __forceinline__ void rapp_int(C (&d)[P], R inv_sat) {
#pragma unroll
  for (int m = 0; m < P; ++m) {
    const R u = fmar(d[m].x, d[m].x, d[m].y * d[m].y) * inv_sat;
    R up = u;
#pragma unroll
    for (int i = 1; i < IP; ++i) up *= u;
    const R sc = rpow_neg_inv<2 * IP>(R(1) + up);
    d[m] = mkc(d[m].x * sc, d[m].y * sc);
  }
}

// PA on all P samples of a thread: one uniform branch on the kind, then a straight loop.
template <bool COLD_OUT, int P, class C, typename R = real_of<C>>
__device__ __forceinline__ void pa_block(int kind, C (&d)[P], R sat, R sqrt_sat, R inv_sat, R rapp_p, R toi) {
#ifdef MIMO_DIAG_PA_SOFTLIM_ONLY  // ISA inspection only (tools/one_inst.hip): no other PA kinds
  kind = PA_SOFTLIM;
#endif
  if (kind == PA_SOFTLIM) {
#pragma unroll
    for (int m = 0; m < P; ++m) d[m] = pa_apply(PA_SOFTLIM, d[m], sat, sqrt_sat, inv_sat, rapp_p, toi);
  } else if (kind == PA_RAPP && rapp_p == R(3)) {
    rapp_int<3>(d, inv_sat);
  } else if (kind == PA_RAPP && rapp_p == R(2)) {
    rapp_int<2>(d, inv_sat);
  } else if (kind == PA_RAPP) {
#pragma unroll
    for (int m = 0; m < P; ++m) {
      if constexpr (COLD_OUT) d[m] = pa_rapp_general(d[m], inv_sat, rapp_p);
      else d[m] = pa_apply(PA_RAPP, d[m], sat, sqrt_sat, inv_sat, rapp_p, toi);
    }
  } else if (kind == PA_TOI) {
#pragma unroll
    for (int m = 0; m < P; ++m) d[m] = pa_apply(PA_TOI, d[m], sat, sqrt_sat, inv_sat, rapp_p, toi);
  }
}

}  // namespace mimo
