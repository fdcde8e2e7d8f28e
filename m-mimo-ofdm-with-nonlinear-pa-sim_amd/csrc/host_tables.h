// Host-built tables of the fused trial kernel: FFT twiddles (team, split and wave-split
// plans), the cot-tan constants, the fp64 Box-Muller tables and the per-point Bussgang-gain
// fits.  One source for the engine (engine.hip ensure_device / fill_point) and for the
// accuracy probe (probe.hip), so that tests see exactly the tables the kernels run on.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "real.h"
#include "alpha_fit.h"
// (the FFT headers for their constexpr layout functions alone: fft_tw_off, ct_rows, wave_fft_fw ...)
#include "team_fft.h"
#include "wave_fft.h"
#include "split_fft.h"

namespace mimo {

// Bussgang gain of modulation.py:178-189 as a function of gamma^2.
inline double alpha_exact(double g2) {
  const double g = std::sqrt(g2);
  return 1.0 - std::exp(-g2) + 0.88622692545275801 * g * std::erfc(g);
}

// Degree-8 fit of alpha(g0^2 / (1 + x)) on |x| <= 0.25 (x = relative deviation of an
// antenna's precoding power from its mean S/A, a few % for MRT): Chebyshev interpolation
// at 64 nodes, converted to monomials in x for a Horner evaluation in fp32.  Max relative
// error ~1e-7 for IBO in [-10, 30] dB (fp32 rounding level); the kernel falls back to
// the exact formula outside the interval.
struct AlphaFit {
  double apoly[9];   // fp32 Horner monomials in x
  double xlim;
  double amono[19];  // fp64 Horner monomials in x (degree 18)
};

inline AlphaFit fit_alpha(double g0sq) {
  AlphaFit p{};
  constexpr int N = 64, D = 8;
  constexpr double L = 0.25;
  double c[D + 1] = {0};
  for (int j = 0; j < N; ++j) {
    const double th = M_PI * (j + 0.5) / N, t = std::cos(th);
    const double f = alpha_exact(g0sq / (1.0 + L * t));
    for (int k = 0; k <= D; ++k) c[k] += f * std::cos(k * th) * (k == 0 ? 1.0 : 2.0) / N;
  }
  // Chebyshev -> monomials in t (T_{k+1} = 2 t T_k - T_{k-1}), then t = x / L
  double Tm1[D + 1] = {0}, T0[D + 1] = {0}, mono[D + 1] = {0};
  T0[0] = 1.0;
  for (int k = 0; k <= D; ++k) {
    for (int i = 0; i <= D; ++i) mono[i] += c[k] * T0[i];
    double Tn[D + 1] = {0};
    for (int i = 0; i <= D; ++i) {
      if (i > 0) Tn[i] += (k == 0 ? 1.0 : 2.0) * T0[i - 1];  // T_1 = t
      Tn[i] -= Tm1[i];
    }
    for (int i = 0; i <= D; ++i) {
      Tm1[i] = T0[i];
      T0[i] = Tn[i];
    }
  }
  double sc = 1.0;
  for (int i = 0; i <= D; ++i, sc /= L) p.apoly[i] = mono[i] * sc;
  p.xlim = L;
  // fp64: Chebyshev interpolant of degree 18 on the same interval at 64 nodes, in long
  // double, converted to monomials in x (Horner in the kernel: 18 FMAs with the
  // coefficients in SGPRs, instead of Clenshaw's 36 ops).  The Taylor radius is 4
  // half-widths (the pole of g0^2 / (1 + x) at x = -1), so the monomials stay O(1) and
  // the Horner sum is as accurate as Clenshaw: <= 1.6e-16 relative against the long
  // double formula over 2e6 points for IBO -5 ... 30 dB (the Clenshaw form: <= 2.1e-16).
  constexpr int D64 = 18;
  long double ck[D64 + 1];
  for (int k = 0; k <= D64; ++k) {
    long double s = 0.0L;
    for (int j = 0; j < N; ++j) {
      const long double th = 3.14159265358979323846264338327950288L * (j + 0.5L) / N;
      const long double t = std::cos(th);
      const long double g2 = (long double)g0sq / (1.0L + (long double)L * t);
      const long double g = std::sqrt(g2);
      const long double f = 1.0L - std::exp(-g2) + 0.886226925452758013649083741671L * g * std::erfc(g);
      s += f * std::cos(k * th);
    }
    ck[k] = s * (k == 0 ? 1.0L : 2.0L) / N;
  }
  long double Um1[D64 + 1] = {0}, U0[D64 + 1] = {0}, um[D64 + 1] = {0};
  U0[0] = 1.0L;
  for (int k = 0; k <= D64; ++k) {
    for (int i = 0; i <= D64; ++i) um[i] += ck[k] * U0[i];
    long double Un[D64 + 1] = {0};
    for (int i = 0; i <= D64; ++i) {
      if (i > 0) Un[i] += (k == 0 ? 1.0L : 2.0L) * U0[i - 1];
      Un[i] -= Um1[i];
    }
    for (int i = 0; i <= D64; ++i) {
      Um1[i] = U0[i];
      U0[i] = Un[i];
    }
  }
  long double scl = 1.0L;
  for (int i = 0; i <= D64; ++i, scl /= (long double)L) p.amono[i] = (double)(um[i] * scl);
  return p;
}

// fp64 Box-Muller tables (real.h ln_unit / sincos_lut), computed in long double, followed
// by the Bussgang-gain segment table (alpha_fit.h; stays in HBM, the kernel copies only the
// first kLut64 entries into LDS).
constexpr int kLut64Alloc = kLut64 + (kAlphaTabDoubles + 1) / 2;
inline std::vector<double2> lut64_table() {
  std::vector<double2> t(kLut64Alloc);
  {
    const std::vector<double> at = alpha_segment_table();
    double* dst = reinterpret_cast<double*>(t.data() + kLut64);
    for (int i = 0; i < kAlphaTabDoubles; ++i) dst[i] = at[i];
  }
  {  // real.h ln_unit: bucket i = m in [0.5 + i 2^-10, 0.5 + (i + 1) 2^-10), c = 1 for the top one
    for (int i = 0; i < kLnTab; ++i) {
      double c = 1.0;
      if (i != kLnTab - 1) {
        const long double ctr = 0.5L + (i + 0.5L) / 1024.0L;
        int ex;
        const long double fr = std::frexp(1.0L / ctr, &ex);
        c = (double)std::ldexp(std::round(std::ldexp(fr, 12)), ex - 12);
      }
      t[i] = make_double2(c, (double)(-std::log((long double)c)));
    }
  }
  for (int i = 0; i < kScTab; ++i) {
    const long double a = 2.0L * 3.14159265358979323846264338327950288L * i / kScTab;
    t[kLnTab + i] = make_double2((double)std::cos(a), (double)std::sin(a));
  }
  return t;
}

// exp(j 2 pi rev) in long double for an angle in revolutions (every angle here is a dyadic
// fraction, so the reduction to [0, 1) is exact).  The tables were first built with the angle
// -2 pi e / F formed in double: its rounding alone (up to 7e-16 near a full turn) put the
// float64 entries up to 2.9 ulp(1) from the true values (tests/test_probe_tables.py); formed in
// long double they are the correctly rounded values but for a 2^-11 ulp.
inline void cis_rev(long double rev, long double& c, long double& s) {
  rev -= std::floor(rev);
  const long double a = 2.0L * 3.14159265358979323846264338327950288L * rev;
  c = std::cos(a);
  s = std::sin(a);
}

// Long-double (cos, sin) -> the table's element: one rounding per component.  ct: the cot-tan
// pair (c, t) with t = sin / c for the *rounded* c, so that the product c t the butterflies
// form is sin to half an ulp (c is never 0: the long-double cos of a quarter turn is 2.5e-20).
struct TwToF32 {
  float2 operator()(long double c, long double s) const { return make_float2((float)c, (float)s); }
  float2 ct(long double c, long double s) const {
    const float cr = (float)c;
    return make_float2(cr, (float)(s / (long double)cr));
  }
};
struct TwToF64 {
  double2 operator()(long double c, long double s) const { return make_double2((double)c, (double)s); }
  double2 ct(long double c, long double s) const {
    const double cr = (double)c;
    return make_double2(cr, (double)(s / (long double)cr));
  }
};

// team-FFT stage twiddles per team size (team_fft.h plan), computed in long double:
// stage s, entry [r][jm] = exp(-j 2 pi e / F) with e = jm r F / (NS R)
template <class Cvt>
inline auto twiddles_of(int F, int T, Cvt cvt) {
  const int P = F / T;
  using V = decltype(cvt(0.0L, 0.0L));
  std::vector<V> tw(std::max(1, fft_tw_total(F, P)), cvt(0.0L, 0.0L));
  for (int st = 1; st < fft_nst(F, P); ++st) {
    const int NS = 1 << fft_bits_before(F, P, st), R = 1 << fft_bits(F, P, st);
    V* blk = tw.data() + fft_tw_off(F, P, st);
    for (int r = 0; r < R; ++r)
      for (int jm = 0; jm < NS; ++jm) {
        const long e_idx = (long)jm * r * (F / (NS * R));
        long double c, sn;
        cis_rev(-(long double)e_idx / (long double)F, c, sn);
        blk[r * NS + jm] = cvt(c, sn);
      }
  }
  return tw;
}

// cot-tan constants of the twiddled stages (team_fft.h dft8_ct / dft16_ct), appended to a
// stage table: (cos a, tan a) per (stage, row, lane); the stored cos is never exactly 0
// (TwToF64::ct), so tan stays finite
// (appended for every instance; the kernels that do not run cot-tan stages never read them)
template <class V, class Cvt>
inline void append_ct(std::vector<V>& tw, int Fs, int P, Cvt cvt) {
  for (int st = 1; st < fft_nst(Fs, P); ++st) {
    const int NS = 1 << fft_bits_before(Fs, P, st), R = 1 << fft_bits(Fs, P, st);
    for (int q = 0; q < ct_rows(R); ++q)
      for (int jm = 0; jm < NS; ++jm) {
        long double c, sn;
        cis_rev((long double)ct_rev(R, NS, jm, q), c, sn);
        tw.push_back(cvt.ct(c, sn));
      }
  }
}

// The team FFT's table of (F, T): the stage twiddles, then the cot-tan region.
template <class Cvt>
inline auto team_twiddles(int F, int T, Cvt cvt) {
  auto tw = twiddles_of(F, T, cvt);
  tw.resize(std::max(1, fft_tw_total(F, F / T)));
  if (F / T >= 2) append_ct(tw, F, F / T, cvt);
  return tw;
}

// split FFT (split_fft.h): the F/2-point sub-transform's table, its cot-tan region, then
// the radix-2 stage's (cos a, tan a), a = -2 pi n / F, n < F/2.  At n = F/4 the pair is
// (-2.5e-20, 4e19): c t rounds to sin a, and the product form c (u.x - t u.y) keeps full
// precision there (tests/test_fft_split.py, near the quarter turn)
inline std::vector<double2> split_twiddles(int F, int T) {
  const int P = F / T;
  const TwToF64 to_f64;
  std::vector<double2> tw64 = twiddles_of(F / 2, T / 2, to_f64);
  tw64.resize(fft_tw_total(F / 2, P));
  if (kSplitCt) append_ct(tw64, F / 2, P, to_f64);
  for (int n = 0; n < F / 2; ++n) {
    long double c, sn;
    cis_rev(-(long double)n / (long double)F, c, sn);
    tw64.push_back(to_f64.ct(c, sn));
  }
  return tw64;
}

// wave-split FFT (wave_fft.h): the one-wave sub-transform's stages, then exp(-j 2 pi n / F)
template <class Cvt>
inline auto wave_twiddles(int F, int T, Cvt cvt) {
  auto tw = twiddles_of(wave_fft_fw(F, T), 64, cvt);
  tw.resize(wave_fft_tw_inter(F, T));
  for (int n = 0; n < F; ++n) {
    long double c, sn;
    cis_rev(-(long double)n / (long double)F, c, sn);
    tw.push_back(cvt(c, sn));
  }
  append_ct(tw, wave_fft_fw(F, T), F / T, cvt);  // the sub-transforms' cot-tan region
  return tw;
}

}  // namespace mimo
