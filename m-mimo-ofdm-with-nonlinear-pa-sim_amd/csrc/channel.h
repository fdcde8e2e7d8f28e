// The channel of the trial kernel, regenerated per antenna at a thread's slots instead of stored:
// Rayleigh draws from Philox (and their power-only and polar forms for pass 1), the closed-form LoS
// and two-path channels, and the caller's table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "real.h"
#include "philox.h"
#include "wave_fft.h"
#include "trial_params.h"
#include "slots.h"

namespace mimo {

// ---------------------------------------------------------------- channel generation
// sin / cos of a channel phase in revolutions: fp32 hardware (v_sin / v_cos take
// revolutions), fp64 the table form (real.h sincos_rev_lut).
__device__ __forceinline__ void sincos_phase(float r, float& sn, float& cs) {
  sn = sin_rev(r);
  cs = cos_rev(r);
}
__device__ __forceinline__ void sincos_phase(double r, double& sn, double& cs) {
  sincos_rev_lut(r, sn, cs);
}

template <typename R, int F, int T, int NSLOT, bool ALIGNED, int CH, bool UNI_EXTRA = false>
struct Channel {
  // philox.h UNI rounds (the rounds whose words are uniform across the team on the SALU): the
  // fp64 wave-split instances (F <= 2048), and UNI_EXTRA (the F 4096 CSI instance, below)
  static constexpr bool kUni = sizeof(R) == 8 && (wave_fft_used(F, T, true) || UNI_EXTRA);
  using SL = Slots<F, T, NSLOT, ALIGNED>;
  using C = cx<R>;
  using Params = TrialParams<R>;

  // CN(0,1) draws of one stream for the thread's slots (pairs resolved in-thread when aligned).
  // c = bm_c(scale^2) scales the draws (box_muller).
  static __device__ __forceinline__ void normals(Key key, uint32_t trial, uint32_t stream, uint32_t aux, int t, int S,
                                                 C (&z)[NSLOT], R c = bm_c<R>(R(1))) {
    if constexpr (ALIGNED) {
      // Pair indices in closed form (pair_of() applied to the aligned slot map):
      //   positive band, slots j and j + Q: q = S/4 - 1 + t + T j, except thread 0 /
      //   j = 0 (bins S/2 and S/4): q = S/2 - 1 with the two draws swapped;
      //   negative band, slots HALF + j and HALF + j + Q: q = t + T j.
      constexpr int Q = SL::HALF / 2;
      const bool t0 = (t == 0);
      const int qp = (S >> 2) - 1 + t;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        C z1, z2;
        const bool sw = (j == 0) && t0;
        cn_pair<kUni>(key, sw ? (uint32_t)((S >> 1) - 1) : (uint32_t)(qp + T * j), trial, stream, aux, z1, z2, c, sw);
        z[j] = z1;
        z[j + Q] = z2;
        cn_pair<kUni>(key, (uint32_t)(t + T * j), trial, stream, aux, z1, z2, c);
        z[SL::HALF + j] = z1;
        z[SL::HALF + j + Q] = z2;
      }
    } else {
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        bool v;
        const int k = SL::k_of(s, t, S, v);
        z[s] = czero<R>();
        if (v) {
          uint32_t q;
          int slot;
          pair_of(k, S, q, slot);
          C z1, z2;
          cn_pair<kUni>(key, q, trial, stream, aux, z1, z2, c);
          z[s] = slot == 0 ? z1 : z2;
        }
      }
    }
  }

  // One Philox call's worth of normals() (aligned instances): chunk c = 2 j + band fills
  // slots (j, j + Q) of the positive band (band 0) or (HALF + j, HALF + j + Q) of the
  // negative band (band 1).  normals() == all 2 Q chunks.
  static constexpr int kChunks = ALIGNED ? SL::HALF : 0;
  static __device__ __forceinline__ void normals_chunk(int c, Key key, uint32_t trial, uint32_t stream, uint32_t aux,
                                                       int t, int S, C (&z)[NSLOT], R cs) {
    if constexpr (ALIGNED) {
      constexpr int Q = SL::HALF / 2;
      const int j = c >> 1;
      C z1, z2;
      if ((c & 1) == 0) {
        const bool sw = (j == 0) && (t == 0);
        cn_pair<kUni>(key, sw ? (uint32_t)((S >> 1) - 1) : (uint32_t)((S >> 2) - 1 + t + T * j), trial, stream, aux, z1, z2,
                cs, sw);
        z[j] = z1;
        z[j + Q] = z2;
      } else {
        cn_pair<kUni>(key, (uint32_t)(t + T * j), trial, stream, aux, z1, z2, cs);
        z[SL::HALF + j] = z1;
        z[SL::HALF + j + Q] = z2;
      }
    }
  }

  // |H|^2 of antenna a at the thread's slots (Rayleigh, FSPL factor f_rel left out as in
  // gen<false>): the same draws as gen(), magnitudes only.
  template <class PP>
  static __device__ __forceinline__ void power(const PP& p, Key key, uint32_t trial, int a, int t,
                                               R (&e2)[NSLOT]) {
    const int S = p.n_sc;
    const R sa = p.ant_rel[a];
    const R c = bm_c<R>(sa * sa);
    if constexpr (ALIGNED) {
      constexpr int Q = SL::HALF / 2;
      const bool t0 = (t == 0);
      const int qp = (S >> 2) - 1 + t;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        R p1, p2;
        const bool sw = (j == 0) && t0;
        cn_pair_pow<kUni>(key, sw ? (uint32_t)((S >> 1) - 1) : (uint32_t)(qp + T * j), trial, ST_CHAN, (uint32_t)a, p1, p2,
                    c, sw);
        e2[j] = p1;
        e2[j + Q] = p2;
        cn_pair_pow<kUni>(key, (uint32_t)(t + T * j), trial, ST_CHAN, (uint32_t)a, p1, p2, c);
        e2[SL::HALF + j] = p1;
        e2[SL::HALF + j + Q] = p2;
      }
    } else {
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        bool v;
        const int k = SL::k_of(s, t, S, v);
        e2[s] = R(0);
        if (v) {
          uint32_t q;
          int slot;
          pair_of(k, S, q, slot);
          R p1, p2;
          cn_pair_pow<kUni>(key, q, trial, ST_CHAN, (uint32_t)a, p1, p2, c);
          e2[s] = slot == 0 ? p1 : p2;
        }
      }
    }
  }

  // power() summed over the antennas in place (pass 1 of the aligned fp64 instances, tuning.h
  // P1_HOIST / P1_SUMS3): acc[.][slot] takes antenna a's term of every slot.
  // SUMS3: the logs stay in real.h ln_unit_parts' three terms, acc[0..2][s] += c (tab, poly, e)
  // (ln_sum() assembles them once per trial); else acc[0][s] += c ln u as power() and its caller.
  // SWAP = false: no pair swap, and q0 is the first call's counter for j = 0, formed by the caller
  // once per trial (S/2 - 1 for thread 0, else S/4 - 1 + t): thread 0's sums of slots 0 and Q
  // then sit in each other's place, which the caller puts right once after the loop.
  // LN_DEG: the degree of the logs' series (real.h ln_unit; tuning.h MIMO_P1_LN_DEG).
  template <bool SUMS3, bool SWAP, int LN_DEG, class PP>
  static __device__ __forceinline__ void power_acc(const PP& p, Key key, uint32_t trial, int a, int t, uint32_t q0,
                                                   R (&acc)[SUMS3 ? 3 : 1][NSLOT]) {
    static_assert(ALIGNED && sizeof(R) == 8, "aligned fp64 instances");
    constexpr int Q = SL::HALF / 2;
    const int S = p.n_sc;
    const R sa = p.ant_rel[a];
    const R c = bm_c<R>(sa * sa);
    const bool t0 = (t == 0);
    const int qp = (S >> 2) - 1 + t;
    auto add = [&](int s, uint32_t w0) __attribute__((always_inline)) {
      if constexpr (SUMS3) {
        R tab, poly, de;
        ln_unit_parts<-32, LN_DEG>((double)w0 + 0.5, tab, poly, de);
        acc[0][s] = fmar(c, tab, acc[0][s]);
        acc[1][s] = fmar(c, poly, acc[1][s]);
        acc[2][s] = fmar(c, de, acc[2][s]);
      } else {
        acc[0][s] += c * bm_log<LN_DEG>(w0, R(0));
      }
    };
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const bool sw = SWAP && (j == 0) && t0;
      uint32_t q = (uint32_t)(qp + T * j);
      if (j == 0) q = SWAP ? (t0 ? (uint32_t)((S >> 1) - 1) : q) : q0;
      uint4 w = philox4x32_10<kUni>(make_uint4(q, trial, ST_CHAN, (uint32_t)a), key);
      add(j, sw ? w.z : w.x);
      add(j + Q, sw ? w.x : w.z);
      w = philox4x32_10<kUni>(make_uint4((uint32_t)(t + T * j), trial, ST_CHAN, (uint32_t)a), key);
      add(SL::HALF + j, w.x);
      add(SL::HALF + j + Q, w.z);
    }
  }

  // Polar form of normals() (aligned instances): rho^2 = c ln u1 and the angle word w1 of
  // every slot's draw (the draw is rho e^{j 2 pi w1 2^-32}, box_muller), no sqrt / sin / cos.
  // fn(slot, rho^2, angle word) per slot, one Philox call (two slots) at a time.
  template <class Fn>
  static __device__ __forceinline__ void polar(Key key, uint32_t trial, uint32_t stream, uint32_t aux, int t, int S, R c,
                                               const Fn& fn) {
    static_assert(ALIGNED, "aligned slot map");
    constexpr int Q = SL::HALF / 2;
    const bool t0 = (t == 0);
    const int qp = (S >> 2) - 1 + t;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const bool sw = (j == 0) && t0;
      uint4 w = philox4x32_10<kUni>(make_uint4(sw ? (uint32_t)((S >> 1) - 1) : (uint32_t)(qp + T * j), trial, stream, aux),
                                    key);
      fn(j, c * bm_log(sw ? w.z : w.x, R(0)), sw ? w.w : w.y);
      fn(j + Q, c * bm_log(sw ? w.x : w.z, R(0)), sw ? w.y : w.w);
      w = philox4x32_10<kUni>(make_uint4((uint32_t)(t + T * j), trial, stream, aux), key);
      fn(SL::HALF + j, c * bm_log(w.x, R(0)), w.y);
      fn(SL::HALF + j + Q, c * bm_log(w.z, R(0)), w.w);
    }
  }

  // normals() with a per-slot scale folded into the Box-Muller radius: z = (rho w_s) e^{j phi}
  // and rw = rho w_s (aligned instances) -- one multiply per draw instead of two.
  // LN_DEG, SIN_DEG: the degrees of the draws' series (real.h ln_unit, sincos_lut; tuning.h
  // MIMO_BM_LN_DEG, MIMO_BM_SIN_DEG).
  template <int LN_DEG = 6, int SIN_DEG = 7>
  static __device__ __forceinline__ void normals_w(Key key, uint32_t trial, uint32_t stream, uint32_t aux, int t, int S,
                                                   R c, const R (&w)[NSLOT], C (&z)[NSLOT], R (&rw)[NSLOT]) {
    static_assert(ALIGNED, "aligned slot map");
    constexpr int Q = SL::HALF / 2;
    const bool t0 = (t == 0);
    const int qp = (S >> 2) - 1 + t;
    auto draw = [&](int s, uint32_t w0, uint32_t w1) __attribute__((always_inline)) {
      rw[s] = sqrt_n1(c * bm_log<LN_DEG>(w0, R(0))) * w[s];
      R sn, cs;
      sincos_lut<SIN_DEG>(w1, sn, cs);
      z[s] = mkc(rw[s] * cs, rw[s] * sn);
    };
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const bool sw = (j == 0) && t0;
      uint4 u = philox4x32_10<kUni>(make_uint4(sw ? (uint32_t)((S >> 1) - 1) : (uint32_t)(qp + T * j), trial, stream, aux),
                                    key);
      draw(j, sw ? u.z : u.x, sw ? u.w : u.y);
      draw(j + Q, sw ? u.x : u.z, sw ? u.y : u.w);
      u = philox4x32_10<kUni>(make_uint4((uint32_t)(t + T * j), trial, stream, aux), key);
      draw(SL::HALF + j, u.x, u.y);
      draw(SL::HALF + j + Q, u.z, u.w);
    }
  }

  // |H|^2 of antenna a at the thread's slots for the closed-form channels (gen<false>'s
  // magnitudes, for pass 1's MRT norms): LoS |a1 e^{j phi1}|^2 = a1^2 -- no phase at all;
  // two-path |a1 e^{j phi1} - a2 e^{j phi2}|^2 = (a1 - a2)^2 + 4 a1 a2 sin^2((phi1 - phi2) / 2)
  // -- one sine of the half path difference instead of two sine / cosine pairs, in the
  // cancellation-free form: a2 / a1 = d_los / d_sec is within ~1e-3 of 1 for the reference's
  // geometry, so at a reflection null (aligned across a ULA) the true value sits near
  // (a1 - a2)^2 ~ 1e-7 a1^2, below the rounding of a1^2 + a2^2 - 2 a1 a2 cos in fp32.  The
  // difference a1 - a2 is formed in fp64 and the half phase reduced to [-1/4, 1/4] rev first.
  template <class PP>
  static __device__ __forceinline__ void power_closed(const PP& p, int a, int t, const double (&rx)[3],
                                                      R (&e2)[NSLOT]) {
    static_assert(CH == CH_LOS || CH == CH_TWOPATH, "closed-form channels");
    const int S = p.n_sc;
    const double tx = p.tx_pos[3 * a], ty = p.tx_pos[3 * a + 1], tz = p.tx_pos[3 * a + 2];
    const double dx = tx - rx[0], dy = ty - rx[1], dz = tz - rx[2];
    const double d_los = sqrt(dx * dx + dy * dy + dz * dz);
    const R att_los = (R)(p.d0 / d_los);
    if constexpr (CH == CH_LOS) {
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        bool v;
        SL::k_of(s, t, S, v);
        e2[s] = v ? att_los * att_los : R(0);
      }
    } else {
      const double hz = tz + rx[2];
      const double d_sec = sqrt(dx * dx + dy * dy + hz * hz);
      const double g_sec = p.d0 / d_sec;
      const R d12 = (R)(p.d0 / d_los - g_sec);
      const R a4 = R(4) * att_los * (R)g_sec;
      const R d12sq = d12 * d12;
      const double dd = d_los - d_sec;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        bool v;
        const int k = SL::k_of(s, t, S, v);
        R e = R(0);
        if (v) {
          double ph = dd * p.f_over_c[k];
          ph -= rint(ph);  // [-1/2, 1/2] rev: the half phase keeps its relative precision
          R sn, cs;
          sincos_phase((R)(0.5 * ph), sn, cs);
          e = fmar(a4 * sn, sn, d12sq);
        }
        e2[s] = e;
      }
    }
  }

  // True channel of antenna a at the thread's slots (relative scale: common factors
  // cancel in MRT, AGC and the SNR normalisation).  FREL = false leaves out the
  // per-sub-carrier FSPL factor fc/f_k, which the kernel then applies once per trial
  // (it cancels in the MRT precoder; see the kernel's AWGN step).
  template <bool FREL, class PP>
  static __device__ __forceinline__ void gen(const PP& p, Key key, uint32_t trial, int a, int t,
                                             const double (&rx)[3], C (&h)[NSLOT]) {
    const int S = p.n_sc;
    if constexpr (CH == CH_RAYLEIGH) {
      const R sa = p.ant_rel[a];
      if (MIMO_ABL(p, ABL_RNG)) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s)
          h[s] = mkc(sa + R(1e-3) * (R)((a + s + t) & 7), R(0.5) - R(1e-3) * (R)((a * s) & 3));
      } else {
        normals(key, trial, ST_CHAN, (uint32_t)a, t, S, h, bm_c<R>(sa * sa));  // ant_rel folded in
      }
      if constexpr (FREL) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
          bool v;
          const int k = SL::k_of(s, t, S, v);
          h[s] = cscale(h[s], v ? p.f_rel[k] : R(0));
        }
      }
    } else if constexpr (CH == CH_TABLE) {
      // the caller's channel (Link.simulate reroll_chan=False), entry `trial` of the bank (the
      // kernel's ch_trial): coalesced loads of the in-band row (f_rel is 1 for table engines:
      // nothing is factored out).  The bank holds at most 2^27 values: the index fits 32 bits.
      const size_t row = ((size_t)trial * (size_t)p.n_ant + (size_t)a) * (size_t)S;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        bool v;
        const int k = SL::k_of(s, t, S, v);
        h[s] = v ? p.chan_tab[row + k] : czero<R>();
      }
    } else {
      const double tx = p.tx_pos[3 * a], ty = p.tx_pos[3 * a + 1], tz = p.tx_pos[3 * a + 2];
      const double dx = tx - rx[0], dy = ty - rx[1], dz = tz - rx[2];
      const double d_los = sqrt(dx * dx + dy * dy + dz * dz);
      const R att_los = (R)(p.d0 / d_los);
      double d_sec = 0.0;
      R att_sec = R(0);
      if constexpr (CH == CH_TWOPATH) {
        // channel.py:138-147: elevation from the mirrored geometry, d_sec = tz/sin(el) +
        // rz/sin(el) with el = atan((tz + rz) / horiz), i.e. the mirrored path length
        // sqrt(horiz^2 + (tz + rz)^2) (no fp64 atan / sin; equal to ~1e-16 relative)
        const double hz = tz + rx[2];
        d_sec = sqrt(dx * dx + dy * dy + hz * hz);
        att_sec = (R)(p.d0 / d_sec);
      }
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        bool v;
        const int k = SL::k_of(s, t, S, v);
        C hv = czero<R>();
        if (v) {
          const double foc = p.f_over_c[k];
          const R fr = FREL ? p.f_rel[k] : R(1);
          double ph = d_los * foc;
          ph -= floor(ph);
          const R a1 = att_los * fr;
          R sn, cs;
          sincos_phase((R)ph, sn, cs);
          hv = mkc(a1 * cs, a1 * sn);
          if constexpr (CH == CH_TWOPATH) {
            double ph2 = d_sec * foc;
            ph2 -= floor(ph2);
            const R a2 = att_sec * fr;
            sincos_phase((R)ph2, sn, cs);
            hv.x -= a2 * cs;
            hv.y -= a2 * sn;
          }
        }
        h[s] = hv;
      }
    }
  }
};

}  // namespace mimo
