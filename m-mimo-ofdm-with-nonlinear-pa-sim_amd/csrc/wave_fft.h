// Wave-split team FFT for the fused trial kernel (gfx950; the instances wave_fft_used() names).
//
// Same contract as TeamFft (team_fft.h): T threads, P = F / T points per thread, the
// frequency-domain vector in the CYCLIC layout (bin e at thread e % T, register e / T),
// un-normalised transforms, run<+1> = frequency -> time, run_second<-1> = time ->
// frequency.  Only the time-domain layout differs, and the PA between the two
// transforms is pointwise.
//
// Four-step split F = WV x FW over the team's WV = T / 64 waves (FW = 64 P):
//   bin k = n2 + FW n1, time n = k1 + WV k2 (n2, k2 < FW; n1, k1 < WV)
//   inverse:  A[k1, n2] = sum_n1 X[n2 + FW n1] e^{+j 2pi n1 k1 / WV}    (in registers)
//             A'        = A e^{+j 2pi k1 n2 / F}
//             x[k1 + WV k2] = sum_n2 A'[k1, n2] e^{+j 2pi n2 k2 / FW}  (wave k1, one wave)
//   forward:  the mirror image (the wave-local FW-point transforms first).
// Thread t holds n2 = t + T i (i < NB = P / WV) for every n1: registers i + NB n1 of the
// cyclic layout.  The radix-WV step is the only one that crosses waves; the FW-point
// transforms (TeamFft<FW, 64, WAVE>) exchange through the wave's own LDS row with no
// hardware barrier.  One s_barrier per transform instead of one or two per exchange.
//
// LDS: WV rows of TeamFft<FW, 64>::LDS_ELEMS (the wave-local exchanges' padded buffer);
// the cross-wave step uses row k1 / row w unpadded.  Thread t writes and reads only the
// cross-wave cells [row][t + T i], so the next transform's cross-wave write needs no
// barrier before it (each thread rewrites exactly the cells it read itself), and a wave's
// row is touched by other waves only inside the cross-wave step, which the barrier
// brackets.
//
// Twiddle table (engine.hip): TeamFft<FW, 64>'s stage blocks, then exp(-j 2pi n / F) for
// n < F (the inter-step twiddles, exponents up to (WV - 1)(FW - 1)).
#pragma once
#include "team_fft.h"

namespace mimo {

// The plan needs at least two waves and whole radix-WV butterflies per thread.
constexpr bool wave_fft_ok(int F, int T) {
  return T >= 128 && T % 64 == 0 && (F / T) >= (T / 64) && (F / T) % (T / 64) == 0;
}
// Instances that use it (kernel and engine): fp64 up to F = 2048.  fp32: not used (F = 8192's 8-wave
// teams measured 17.43 -> 17.64 ms with it, profiles/r02/ab/ab_wavefft_8192_f32.json; below
// F = 8192 the 2-wave fp32 teams need only two exchanges per transform, which the split
// would raise to three).
// fp64 config 2: 58.82 -> 58.50 ms (profiles/r02/ab/ab_wavefft_2048_f64.json).  The
// barriers were not what the exchanges cost: their LDS round trips remain.
constexpr bool wave_fft_used(int F, int T, bool f64) {
  // F 4096 / 8192 run 16-point teams (trial_launch.h team_size64) on the team FFT: the
  // wave-split rows would not leave room for a second team at F 4096, and measured
  // neutral at F 8192 (profiles/r03/ab8k/ab_p16_wave.json).
  return wave_fft_ok(F, T) && f64 && F <= 2048;
}
constexpr int wave_fft_fw(int F, int T) { return F / (T / 64); }
constexpr int wave_fft_tw_inter(int F, int T) { return fft_tw_total(wave_fft_fw(F, T), F / T); }
constexpr int wave_fft_tw_total(int F, int T) { return wave_fft_tw_inter(F, T) + F; }
// The fp64 sub-transforms' cot-tan constants (team_fft.h dft8_ct) follow the inter twiddles
// (fft_ct_n entries).
constexpr int wave_fft_ct_n(int F, int T) { return fft_ct_n(wave_fft_fw(F, T), F / T); }

template <int F, int T, typename Re, bool LTW1 = true, bool LTW2 = LTW1>
struct WaveFft {
  using C = cx<Re>;
  static constexpr int P = F / T;
  static constexpr int WV = T / 64;
  static constexpr int FW = F / WV;
  static constexpr int NB = P / WV;
  static_assert(wave_fft_ok(F, T), "wave-split plan needs >= 2 waves and P a multiple of the wave count");
  // LTW1: stage-1 twiddles from LDS (tw1); from four waves on (F 2048) also stage 2's rows
  // r = 3, 5, 6 (config 2 -0.5 %, LoS -0.8 %, MCNC -1.0 %, profiles/r03/ab_x; at F 1024 the
  // 3 KiB more would cost the third wave per SIMD)
  // fp64 with both LDS twiddle blocks: the twiddled radix-8 stages absorb their twiddles
  // into FMAs (team_fft.h dft8_ct; the constants from the cot-tan region of the table)
  using Sub = TeamFft<FW, 64, 1, Re, true, LTW1, LTW2 && (T / 64) >= 4, sizeof(Re) == 8>;
  static constexpr int TW1_N = Sub::TW1_N;
  static constexpr int TWL_N = Sub::TWL_N;         // tw1: LDS copy of the entries twl_src names
  static __device__ __forceinline__ int twl_src(int i) {
    return Sub::CT ? wave_fft_tw_total(F, T) + i : Sub::twl_src(i);
  }
  static_assert(!Sub::CT || Sub::CT_N == wave_fft_ct_n(F, T), "cot-tan table layout");
  static_assert(Sub::P == P, "sub-transform keeps the points per thread");
  static constexpr int ROW = Sub::LDS_ELEMS;
#ifdef MIMO_DIAG_ROWS2
  // Diagnostic builds only (wrong results): the waves share two exchange rows (row w & 1), so
  // the team's exchange LDS halves -- the occupancy A/B of 4 waves / SIMD at F 2048
  // (profiles/r06/w4/), every access in bounds
  static constexpr int LDS_TOTAL = 2 * ROW;
  static __host__ __device__ constexpr int row_of(int w) { return (w & 1) * ROW; }
#else
  static constexpr int LDS_TOTAL = WV * ROW;
  static __host__ __device__ constexpr int row_of(int w) { return w * ROW; }
#endif
  static constexpr int XCHG = 1 + Sub::XCHG;  // exchange windows per transform (fill calls)
  static constexpr int TW_INTER = wave_fft_tw_inter(F, T);

  // ---- XADDR (tuning.h MIMO_XADDR): the thread's LDS byte addresses, formed once per trial and
  // held two per 32-bit word across the antenna loop, instead of re-derived from the thread id
  // by every transform.  Each is a function of t alone (w = t / 64, l = t % 64), relative to
  // the exchange array (the stage constants: to the LDS twiddle copy tw1):
  //   xa_cross  [row 0][t]: the inverse's cross-wave writes, the forward's reads (+ row k1, T i)
  //   xa_row    [row w][l]: the cross-wave reads / writes of wave w's own row (+ 64 m) and the
  //             sub-transform's stage-0 writes (+ r XS0)
  //   xa_x0r    the transposed exchange 0's read base of the sub-transform (+ (64 / R0) m)
  //   xa_x1w    exchange 1's padded write base (+ pad(r NS))
  //   xa_x1r    exchange 1's read base pad<1>(l) (+ pad(64 m))
  //   xa_tw     lane l of the stage constants' rows: stage 2's base (NS = 64), and masked to
  //             l & (NS - 1) stage 1's
  // The same formulas serve the host mirror (mimo_xaddr_words, tests/test_xaddr_host.py).
  static constexpr int CB = (int)sizeof(C);
  static constexpr bool XA_TW = MIMO_XADDR_TW != 0;
  static __host__ __device__ constexpr uint32_t xa_cross(int t) { return (uint32_t)(CB * t); }
  static __host__ __device__ constexpr uint32_t xa_row(int t) { return (uint32_t)(CB * (row_of(t >> 6) + (t & 63))); }
  static __host__ __device__ constexpr uint32_t xa_x0r(int t) {
    return (uint32_t)(CB * (row_of(t >> 6) + Sub::x0_read(t & 63)));
  }
  static __host__ __device__ constexpr uint32_t xa_x1w(int t) {
    return (uint32_t)(CB * (row_of(t >> 6) + Sub::template x_write<1>(t & 63)));
  }
  static __host__ __device__ constexpr uint32_t xa_x1r(int t) {
    return (uint32_t)(CB * (row_of(t >> 6) + Sub::template pad<1>(t & 63)));
  }
  static __host__ __device__ constexpr uint32_t xa_tw(int t) { return (uint32_t)(CB * (t & 63)); }
  // The largest address a packed half can hold: the last thread's, plus the largest immediate
  // offset of its use, stays inside the exchange array; all are multiples of the element size.
  static constexpr bool XA_PLAN = Sub::NST == 3 && Sub::XP0 && Sub::P == (1 << Sub::bits(0)) && LTW1 &&
                                  (1 << Sub::bits_before(2)) == 64;
  static_assert(!XA_PLAN || ((int64_t)CB * LDS_TOTAL < 65536 && CB % 16 == 0 && CB * TWL_N < 65536),
                "XADDR: every LDS byte address of the team fits 16 bits and is 16-byte aligned");
  struct XAddr {
    static constexpr bool on = true;
    uint32_t w_cr;  // xa_cross | xa_row << 16
    uint32_t w_x;   // xa_x0r | xa_x1w << 16
    uint32_t w_t;   // xa_tw | xa_x1r << 16
    int w;          // the thread's wave, uniform (an SGPR)
    static __host__ __device__ constexpr uint32_t word_cr(int t) { return xa_cross(t) | xa_row(t) << 16; }
    static __host__ __device__ constexpr uint32_t word_x(int t) { return xa_x0r(t) | xa_x1w(t) << 16; }
    static __host__ __device__ constexpr uint32_t word_t(int t) { return xa_tw(t) | xa_x1r(t) << 16; }
    __device__ __forceinline__ void set(int t, int wave) {
      w_cr = word_cr(t);
      w_x = word_x(t);
      w_t = word_t(t);
      w = wave;
    }
    // The held words themselves made opaque, in place (no copy): what is unpacked from them
    // cannot be hoisted out of the caller's antenna loop.
    __device__ __forceinline__ void launder() {
      asm volatile("" : "+v"(w_cr), "+v"(w_x), "+v"(w_t));
    }
    __host__ __device__ constexpr uint32_t cross() const { return w_cr & 0xffffu; }
    __host__ __device__ constexpr uint32_t row() const { return w_cr >> 16; }
    __host__ __device__ constexpr uint32_t x0r() const { return w_x & 0xffffu; }
    __host__ __device__ constexpr uint32_t x1w() const { return w_x >> 16; }
    __host__ __device__ constexpr uint32_t x1r() const { return w_t >> 16; }
    __host__ __device__ constexpr uint32_t tw() const { return w_t & 0xffffu; }
    // stage S's constants: lane l & (NS - 1) of each row (the low half needs no unpack first)
    template <int NS>
    __host__ __device__ constexpr uint32_t tws() const {
      return w_t & (uint32_t)(CB * (NS - 1));
    }
    // XADDR_TW: per-lane byte offsets into the inter-step twiddles exp(-j 2 pi n / F), n < F
    __host__ __device__ constexpr uint32_t tw_inv(int k) const { return (uint32_t)k * cross(); }  // CB k t
    __host__ __device__ constexpr uint32_t tw_fwd(int wv) const { return (uint32_t)(wv & 0xff) * tw(); }  // CB w l
  };
  static __device__ __forceinline__ C* at(C* base, uint32_t boff) {
    return reinterpret_cast<C*>(reinterpret_cast<char*>(base) + boff);
  }
  static __device__ __forceinline__ C gload_b(const C* base, uint32_t boff) { return Sub::gload_b(base, boff); }

  using NoFill = typename Sub::NoFill;
  static __device__ __forceinline__ int freq_thread(int t) { return t; }  // cyclic in t

  // Zero mask of radix-WV butterfly i's inputs v[n1] = d[i + NB n1] from the register mask.
  static constexpr uint32_t bfly_mask(uint32_t zm, int i) {
    uint32_t m = 0;
    for (int n1 = 0; n1 < WV; ++n1) m |= ((zm >> (i + NB * n1)) & 1u) << n1;
    return m;
  }

  // w[k] = exp(-j 2pi k n / F), k = 1 .. WV-1: powers of two loaded, the rest as products.
  static __device__ __forceinline__ void inter_tw(C (&w)[WV], const C* __restrict__ tw, int n) {
#pragma unroll
    for (int k = 1; k < WV; ++k) {
      if ((k & (k - 1)) == 0) {
        w[k] = Sub::gload(tw + TW_INTER, k * n);
      } else {
        int hb = k;
        while (hb & (hb - 1)) hb &= hb - 1;
        w[k] = cmul(w[hb], w[k - hb]);
      }
    }
  }

  // Powers of two below WV (the inter-step twiddles that are loaded), and the uniform table
  // bases of XADDR_TW: entry k T i of the inter-step twiddles for butterfly i and k = 2^b.  Each
  // is formed on the SALU per transform and opaque, so that none is folded back into per-lane
  // 64-bit arithmetic or held in SGPRs across the caller's loop.
  static constexpr int KP = ilog2(WV);
  struct InvBases {
    const C* b[NB][KP];
  };
  static __device__ __forceinline__ void inv_bases(InvBases& ib, const C* tw) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
#pragma unroll
      for (int b = 0; b < KP; ++b) {
        const C* q = tw + TW_INTER + (T * i << b);
        asm("" : "+s"(q));
        ib.b[i][b] = q;
      }
    }
  }
  template <int I, int DIR, uint32_t ZM, class XA = NoXA>
  static __device__ __forceinline__ void inv_butterfly(C (&d)[P], C* lds, const C* __restrict__ tw, int t,
                                                       bool no_xchg, const XA& xa = XA{},
                                                       const InvBases* ib = nullptr) {
    C v[WV];
#pragma unroll
    for (int n1 = 0; n1 < WV; ++n1) v[n1] = d[I + NB * n1];
    Dft<WV, DIR, bfly_mask(ZM, I)>::run(v);
    const int n2 = t + T * I;
    C w[WV];
    if constexpr (XA::on && XA_TW) {
      // entry k n2 = k t + k T I: the lane's part a 32-bit byte offset, the rest in the uniform base
#pragma unroll
      for (int k = 1; k < WV; ++k) {
        if ((k & (k - 1)) == 0) {
          w[k] = gload_b(ib->b[I][ilog2(k)], xa.tw_inv(k));
        } else {
          int hb = k;
          while (hb & (hb - 1)) hb &= hb - 1;
          w[k] = cmul(w[hb], w[k - hb]);
        }
      }
    } else {
      inter_tw(w, tw, n2);
    }
#pragma unroll
    for (int k1 = 1; k1 < WV; ++k1) v[k1] = cmulc(v[k1], w[k1]);  // DIR = +1: e^{+j ...}
    if (no_xchg) {
#pragma unroll
      for (int k1 = 0; k1 < WV; ++k1) d[I + NB * k1] = v[k1];
    } else if constexpr (XA::on) {
      C* wb = at(lds, xa.cross());
#pragma unroll
      for (int k1 = 0; k1 < WV; ++k1) wb[row_of(k1) + T * I] = v[k1];
    } else {
#pragma unroll
      for (int k1 = 0; k1 < WV; ++k1) lds[row_of(k1) + n2] = v[k1];
    }
  }
  template <int DIR, uint32_t ZM, int I = 0, class XA = NoXA>
  static __device__ __forceinline__ void inv_butterflies(C (&d)[P], C* lds, const C* __restrict__ tw, int t,
                                                         bool no_xchg, const XA& xa = XA{},
                                                         const InvBases* ib = nullptr) {
    if constexpr (I < NB) {
      inv_butterfly<I, DIR, ZM>(d, lds, tw, t, no_xchg, xa, ib);
      inv_butterflies<DIR, ZM, I + 1>(d, lds, tw, t, no_xchg, xa, ib);
    }
  }

  // Frequency (cyclic) -> time (wave k1, lane l, register m: n = k1 + WV (l + 64 m)).
  template <int DIR, int PAR = 0, uint32_t ZM = 0, typename Fill = NoFill>
  static __device__ __forceinline__ void run(C (&d)[P], C* lds, const C* __restrict__ tw, int t,
                                             bool no_xchg = false, const Fill& fill = Fill{},
                                             const C* tw1 = nullptr) {
    static_assert(DIR == +1, "run: the inverse (frequency -> time) transform");
    const C* twl = tw;
    int tl = t;
    asm volatile("" : "+s"(twl));
    asm volatile("" : "+v"(tl));
    inv_butterflies<DIR, ZM>(d, lds, twl, tl, no_xchg);
    const int w = tl >> 6, l = tl & 63;
    if (!no_xchg) {
      __syncthreads();
      const C* rb = lds + row_of(w) + l;
#pragma unroll
      for (int m = 0; m < P; ++m) d[m] = rb[64 * m];
    }
    fill(0);
    auto sub_fill = [&](int s) __attribute__((always_inline)) { fill(s + 1); };
    Sub::template run<DIR, 0, 0u>(d, lds + row_of(w), twl, l, no_xchg, sub_fill, tw1);
  }
  // ... with the thread's LDS addresses held by the caller (XADDR): the packed words are what
  // is laundered per transform, t only where the inter-step twiddles still index by it
  // (XA_TW off).
  template <int DIR, int PAR = 0, uint32_t ZM = 0, typename Fill = NoFill>
  static __device__ __forceinline__ void run(C (&d)[P], C* lds, const C* __restrict__ tw, XAddr& xa, int t,
                                             bool no_xchg = false, const Fill& fill = Fill{},
                                             const C* tw1 = nullptr) {
    static_assert(DIR == +1, "run: the inverse (frequency -> time) transform");
    static_assert(XA_PLAN, "XADDR: the three-stage one-wave sub-transform");
    const C* twl = tw;
    asm volatile("" : "+s"(twl));
    xa.launder();
    int tl = 0;
    if constexpr (!XA_TW) {
      tl = t;
      asm volatile("" : "+v"(tl));
    }
    InvBases ib;
    if constexpr (XA_TW) inv_bases(ib, twl);
    inv_butterflies<DIR, ZM>(d, lds, twl, tl, no_xchg, xa, &ib);
    if (!no_xchg) {
      __syncthreads();
      const C* rb = at(lds, xa.row());
#pragma unroll
      for (int m = 0; m < P; ++m) d[m] = rb[64 * m];
    }
    fill(0);
    auto sub_fill = [&](int s) __attribute__((always_inline)) { fill(s + 1); };
    Sub::template run_x<DIR, 0, 0u>(d, lds, twl, no_xchg, sub_fill, tw1, xa);
  }

  // Time (as run() leaves it) -> frequency (cyclic).
  template <int DIR, typename Fill = NoFill>
  static __device__ __forceinline__ void run_second(C (&d)[P], C* lds, const C* __restrict__ tw, int t,
                                                    bool no_xchg = false, const Fill& fill = Fill{},
                                                    const C* tw1 = nullptr) {
    static_assert(DIR == -1, "run_second: the forward (time -> frequency) transform");
    const C* twl = tw;
    int tl = t;
    asm volatile("" : "+s"(twl));
    asm volatile("" : "+v"(tl));
    const int w = tl >> 6, l = tl & 63;
    Sub::template run<DIR, 0, 0u>(d, lds + row_of(w), twl, l, no_xchg, fill, tw1);
    // B'[w, q] = B[w, q] e^{-j 2pi w q / F}, q = l + 64 m (wave-uniform branch)
    // (all P loads issued before the first multiply: one wait instead of P round trips).
    // The products go straight to the exchange row inside the branch: merged back into d
    // after it, they cost P register-pair copies per transform (v_mov_b64 at the join).
    C* wb = lds + row_of(w) + l;
    if (w > 0) {
      C tw[P];
#pragma unroll
      for (int m = 0; m < P; ++m) tw[m] = Sub::gload(twl + TW_INTER, w * (l + 64 * m));
      if (no_xchg) {
#pragma unroll
        for (int m = 0; m < P; ++m) d[m] = cmul(d[m], tw[m]);
      } else {
#pragma unroll
        for (int m = 0; m < P; ++m) wb[64 * m] = cmul(d[m], tw[m]);
      }
    } else if (!no_xchg) {
#pragma unroll
      for (int m = 0; m < P; ++m) wb[64 * m] = d[m];
    }
    if (!no_xchg) __syncthreads();
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      C v[WV];
#pragma unroll
      for (int w2 = 0; w2 < WV; ++w2) v[w2] = no_xchg ? d[i + NB * w2] : lds[row_of(w2) + tl + T * i];
      Dft<WV, DIR>::run(v);
#pragma unroll
      for (int k1 = 0; k1 < WV; ++k1) d[i + NB * k1] = v[k1];
    }
    fill(Sub::XCHG);
  }
  // ... with the held addresses (XADDR), as run() above
  template <int DIR, typename Fill = NoFill>
  static __device__ __forceinline__ void run_second(C (&d)[P], C* lds, const C* __restrict__ tw, XAddr& xa, int t,
                                                    bool no_xchg = false, const Fill& fill = Fill{},
                                                    const C* tw1 = nullptr) {
    static_assert(DIR == -1, "run_second: the forward (time -> frequency) transform");
    const C* twl = tw;
    asm volatile("" : "+s"(twl));
    xa.launder();
    int tl = 0;
    if constexpr (!XA_TW) {
      tl = t;
      asm volatile("" : "+v"(tl));
    }
    Sub::template run_x<DIR, 0, 0u>(d, lds, twl, no_xchg, fill, tw1, xa);
    C* wb = at(lds, xa.row());
    int w = xa.w;  // (its own opaque copy: the bases below are formed per transform, not held)
    asm volatile("" : "+s"(w));
    if (w > 0) {
      C tw[P];
      if constexpr (XA_TW) {
        // entry w (l + 64 m): the lane's w l a 32-bit byte offset, 64 w m in the uniform base
        const C* twb = twl + TW_INTER;
        const uint32_t lo = xa.tw_fwd(w);
#pragma unroll
        for (int m = 0; m < P; ++m) tw[m] = gload_b(twb + w * (64 * m), lo);
      } else {
        const int l = tl & 63;
#pragma unroll
        for (int m = 0; m < P; ++m) tw[m] = Sub::gload(twl + TW_INTER, w * (l + 64 * m));
      }
      if (no_xchg) {
#pragma unroll
        for (int m = 0; m < P; ++m) d[m] = cmul(d[m], tw[m]);
      } else {
#pragma unroll
        for (int m = 0; m < P; ++m) wb[64 * m] = cmul(d[m], tw[m]);
      }
    } else if (!no_xchg) {
#pragma unroll
      for (int m = 0; m < P; ++m) wb[64 * m] = d[m];
    }
    if (!no_xchg) __syncthreads();
    const C* cb = at(lds, xa.cross());
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      C v[WV];
#pragma unroll
      for (int w2 = 0; w2 < WV; ++w2) v[w2] = no_xchg ? d[i + NB * w2] : cb[row_of(w2) + T * i];
      Dft<WV, DIR>::run(v);
#pragma unroll
      for (int k1 = 0; k1 < WV; ++k1) d[i + NB * k1] = v[k1];
    }
    fill(Sub::XCHG);
  }
};

}  // namespace mimo
