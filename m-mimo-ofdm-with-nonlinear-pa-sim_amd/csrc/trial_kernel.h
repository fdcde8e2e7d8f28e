// Fused Monte-Carlo BER trial kernel for gfx950 (MI355X).
//
// One workgroup ("team", T threads) runs one trial = one OFDM symbol of
// mp_model.Link.simulate (mp_model.py:180-222; clean run :133-175) entirely on chip:
//
//   labels (Philox BITS) -> pre-weighted symbols s / ||H|| / sqrt(F) (LDS)   mp_model.py:208
//   pass 1: channel power draws -> MRT norms sum_a |H|^2   antenna_array.py:162-173
//           (Rayleigh: rho^2 = -ln u1 only, no sqrt / sin / cos)
//   pass 3: per antenna a
//       H (Philox CHAN x FSPL, or closed-form LoS/two-path)  channel.py:35-72,116-167,262-275
//       alpha_a from the per-antenna precoding power      mp_model.py:312-326
//       X = s conj(H) / ||H||  -> IFFT -> PA -> FFT       modulation.py:332-361, distortion.py, utilities.py:311-329
//       r += H Y,  g += alpha_a |H|^2 / ||H||             channel.py:287-290, mp_model.py:320-326
//   AWGN (Philox NOISE) scaled by Es eta / snr, z = (r + n)/g   noise.py:56-83, mp_model.py:210-214
//   CNC (corrector.py:52-112) or MCNC (corrector.py:165-207) iterations, hard slicer,
//   XOR-popcount bit errors -> counts[trial][idx]         mp_model.py:215-222
//
// Nothing per trial touches HBM except the final per-trial counts (n_idx x 4 B) and the
// receiver stage's register spills: the channel is regenerated from Philox instead of
// being stored.  Frequency-domain data live in the team FFT's cyclic
// register layout; each thread owns NSLOT in-band sub-carriers ("slots").
//
// Without CSI errors the per-sub-carrier FSPL ratio f_c/f_k is factored out of the
// antenna loops (it cancels in MRT) and the per-antenna ratio is folded into the
// Box-Muller radius; alpha_a comes from a host-fitted polynomial (fp32, F <= 4096) or a
// Chebyshev series (fp64).  Both instances are VALU-issue-bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <type_traits>

#include "tuning.h"
#include "alpha_fit.h"
#include "philox.h"
#include "softbits.h"
#include "team_fft.h"
#include "wave_fft.h"
#include "split_fft.h"
// The kernel's contract and components.  Keep the order: out-of-line device functions (pa.h
// pa_rapp_general) are emitted in the order of their definitions, and tools/isa_identity.py
// compares builds line for line.
#include "trial_params.h"
#include "slots.h"
#include "team_sum.h"
#include "pa.h"
#include "qam.h"
#include "channel.h"

namespace mimo {

// ISA inspection only (tools/stage_hist.py): a comment in the assembly naming the loop.
#ifdef MIMO_ISA_MARKERS
#define MIMO_ISA_MARK(name) asm volatile("; MIMO_MARK " name)
#else
#define MIMO_ISA_MARK(name) ((void)0)
#endif

// bin of a sample power (the envelope instances, trial_params.h MIMO_MODE_ENV):
// clamp((bits(pw scale) >> 49) - 8088, 0, 127), 8088 = (1023 - 12) << 3
// (pw scale >= 0: bits >> 49 is the high word >> 17; 0 lands in bin 0, +inf in bin 127)
__device__ __forceinline__ int env_bin(double pw, double scale) {
  const int b = (__double2hiint(pw * scale) >> 17) - 8088;
  return b < 0 ? 0 : (b > kEnvBins - 1 ? kEnvBins - 1 : b);
}

// ---------------------------------------------------------------- the kernel
// The instance's FFT.  fp64 up to F 2048 on two or more waves: the wave-split FFT (wave_fft.h).
// fp64 F 8192: two 4096-point sub-transforms and a radix-2 stage through lane-half swaps
// (split_fft.h: two LDS exchanges per transform instead of three).  Else the team FFT; fp64 up
// to F 4096 its twiddled stages absorb their twiddles into FMAs (team_fft.h dft8_ct / dft16_ct).
template <typename R, int F, int T, int NBUF>
using trial_fft_t = std::conditional_t<
    wave_fft_used(F, T, sizeof(R) == 8), WaveFft<F, T, R, true, true>,
    std::conditional_t<split_fft_used(F, T, sizeof(R) == 8), SplitFft<F, T, NBUF, R>,
                       TeamFft<F, T, NBUF, R, false, false, false, sizeof(R) == 8 && F <= 4096>>>;

// The held transform addresses of an instance (wave_fft.h XAddr), or nothing.
template <class FFT, bool ON>
struct XAddrOf {
  using type = NoXA;
};
template <class FFT>
struct XAddrOf<FFT, true> {
  using type = typename FFT::XAddr;
};
// Instances that hold them (tuning.h MIMO_XADDR): the fp64 wave-split instances without CSI whose
// scratch does not grow with the three words (profiles/r22/xaddr/resources.txt; one that grows,
// by 16 to 64 B / lane, keeps re-deriving).  Per size and run mode a mask
// over (aligned ? 0 : 4) + channel kind - 1 of the instances left out.
constexpr bool xaddr_inst_ok(int F, int mode, bool aligned, int ch) {
  constexpr unsigned out1024[7] = {0x91, 0x82, 0x81, 0x91, 0x00, 0xD8, 0xD1};
  constexpr unsigned out2048[7] = {0x80, 0x90, 0x00, 0x80, 0x20, 0x40, 0x80};
  if (mode == MIMO_MODE_TURBO) mode = MIMO_MODE_CODED;  // the turbo instances: the coded instances' choices, inherited
  if (mode < 0 || mode > 6 || ch < 1 || ch > 4) return false;
  const unsigned bit = 1u << ((aligned ? 0 : 4) + ch - 1);
  return F == 1024 ? !(out1024[mode] & bit) : F == 2048 ? !(out2048[mode] & bit) : false;
}

// Box-Muller tables (real.h ln_unit / sincos_lut) into LDS, by the whole team; the caller
// barriers before the first read.  p: the kernel parameters, or anything with their `lut`
// (a pointer, not a reference: the table pointer is then loaded where the kernel always
// loaded it, under the loop guard.  The float32 instances' instruction streams are what they
// were before the loop became a function; the float64 ones keep their instruction mix but
// differ in register names, instruction order and the form of a few loop guards, since the
// inlined loop's block lands before the code that follows it).
template <int T, class PP>
__device__ __forceinline__ void fill_lut64(const PP* p, int t) {
  for (int i = t; i < kLut64; i += T) lut64[i] = p->lut[i];
}
// The wave-split sub-transform's LDS twiddle copy (stage 1's block and stage 2's rows, or the
// cot-tan constants; team_fft.h twl_src) from the instance's table; same barrier.  (The
// thread id read here, not passed in: its range keeps the index arithmetic unsigned.)
template <class FFT, int T, class C>
__device__ __forceinline__ void fill_tw1(C* tw1_s, const C* twsrc) {
  for (int i = threadIdx.x; i < FFT::TWL_N; i += T) tw1_s[i] = twsrc[FFT::twl_src(i)];
}

// Occupancy tuning per instance (trial_inst.hip): MINW = waves/SIMD the register
// allocation targets, NBUF = FFT exchange buffers (2: one barrier per exchange, 1: half
// the LDS), SYMW_LDS = keep the pre-weighted symbols in LDS (thread-private) instead of
// registers.  F = 2048 runs (3, 1, true): 25 KiB LDS and <= 168 VGPRs per 128-thread team.
template <int MODE, typename R, int F, int T, int NSLOT, bool ALIGNED, int CH, bool CSI, int MINW, int NBUF, bool SYMW_LDS,
          typename... MA>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(MINW))) void trial_kernel(TrialParams<R> p0, MA... a) {
  static_assert(std::is_same_v<std::tuple<MA...>, ModeArgs<MODE>>, "the kernel's arguments behind p0 are the mode's");
  const ModeArgs<MODE> ma(a...);
  using C = cx<R>;
  constexpr bool MEAS = MODE == MIMO_MODE_MEAS && sizeof(R) == 8;
  constexpr bool SPEC = MODE == MIMO_MODE_SPEC && sizeof(R) == 8;
  constexpr bool BEAM = MODE == MIMO_MODE_BEAM && sizeof(R) == 8;
  constexpr bool ENV = MODE == MIMO_MODE_ENV && sizeof(R) == 8;
  constexpr bool SOFT = MODE == MIMO_MODE_SOFT && sizeof(R) == 8;
  constexpr bool CODED = MODE == MIMO_MODE_CODED && sizeof(R) == 8;
  constexpr bool TURBO = MODE == MIMO_MODE_TURBO && sizeof(R) == 8;
  // ---- which point and trial this block runs (uniform binary search over point_start)
  uint32_t pi = 0;
  if (p0.n_points > 1) {
    uint32_t lo = 0, hi = (uint32_t)p0.n_points;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (p0.point_start[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    pi = lo;
  }
  using CParams = const __attribute__((address_space(4))) TrialParams<R>;
  CParams& p = *(CParams*)(p0.points + pi);
  constexpr bool WAVEFFT = wave_fft_used(F, T, sizeof(R) == 8);
  // The sub-transforms read their twiddled stages' constants from LDS (stage 1's block and
  // stage 2's rows; fp64: the cot-tan constants of dft8_ct).  CSI instances too, since their
  // per-antenna power table is dynamic LDS sized by A (round 5; before, a static 4 KiB
  // table left no room for stage 2's rows at 3 teams per CU).
  // fp64 up to F 4096: the twiddled stages absorb their twiddles into FMAs (team_fft.h
  // dft8_ct / dft16_ct; F 4096 -1.0 to -1.6 %, CSI -7 to -12 %).  F 8192 keeps the stage
  // twiddles with the prefetched bases: the cot-tan form measured +2.5 % there (its 16-point
  // threads hold the extra constants live across the exchanges; profiles/r05/ab/ab_5su_r05e.json).
  // fp64 F 8192: two 4096-point sub-transforms and a radix-2 stage through lane-half swaps
  // (split_fft.h: two LDS exchanges per transform instead of three)
  constexpr bool SPLITFFT = split_fft_used(F, T, sizeof(R) == 8);
  using FFT = trial_fft_t<R, F, T, NBUF>;
  using SL = Slots<F, T, NSLOT, ALIGNED>;
  // F 4096: the SALU Philox rounds with CSI only -- CSI -2.4 %, perfect CSI +1.1 / +2.0 %
  // (paper / paper CNC 0-8, profiles/r06/k4096/; r03 measured +1.7 % for the perfect-CSI line)
  // F 8192: on since round 6 together with the folded weight (below): config-5 array -1.6 %
  // for both, -1.3 % for the weight alone, +0.4 % for these rounds alone (profiles/r06/k8192/;
  // +1.4 % alone in round 3)
  using CHN = Channel<R, F, T, NSLOT, ALIGNED, CH,
                      (F == 4096 && CSI && MIMO_UNI_4096_CSI != 0) || (F == 8192 && MIMO_UNI_8192 != 0)>;
  constexpr int P = FFT::P;
  constexpr int W = T / 64;
  // Without CSI errors the channel factors as H[a,k] = f_rel[k] H'[a,k]: f_rel cancels in
  // the MRT precoder and in vk_pow, scales r and g by f_rel, and enters only through the
  // AGC power eta and the noise term z = r'/g' + sigma n / (f_rel g').  The antenna loops
  // then run on H' (no per-antenna table reads).  With CSI the estimate's error power
  // mixes sub-carriers, so H keeps the factor.
  constexpr bool FREL = CSI;

  __shared__ C lds[FFT::LDS_TOTAL];
  __shared__ R red[T / 64];  // sized by the team
  __shared__ R vk_part[2][T / 64];
  // alpha formed by one wave per antenna (array_pass): config 2 -1.0 %, CSI -1.2 %, config-5
  // array -2.3 % (profiles/r05/ab/ab_*_alpha1.json).  MIMO_ALPHA1=0: every wave forms it.
  // F 4096 (fp64) since round 6, with the cold paths out of line there: -0.1 % alone, and
  // -1.4 % / -1.0 % together with them (profiles/r06/k4096/; alone +0.8 % in round 5)
  constexpr bool ALPHA1 = MIMO_ALPHA1 != 0 && (F != 4096 || (MIMO_ALPHA1_4096 != 0 && sizeof(R) == 8));
  __shared__ R alpha_s[2];
  // VK_LDS (tuning.h; fp64 wave-split instances without CSI): the waves hand their vk partials
  // over per thread, one ds_write_b64 each in place of the DPP tree, and the alpha wave of the
  // antenna adds them per lane to its own (kept in registers) and runs the one tree.  W - 1
  // regions of 64 partials.  With a fixed alpha wave k (ALPHA_WAVE below) wave w's region is a
  // compile-time function of w, w - (w > k), and the alpha wave adds the W partials in wave order
  // 0, 1, ..., its own in its place, so alpha does not depend on the antenna's index.  With the
  // alpha wave rotating (a mod W) the regions rotate with it: wave w writes region
  // (w - a - 1) mod W.
  // (1.5 KiB at T 256: the F 2048 instance's LDS 51,824 -> 53,296 B, and three teams per CU are
  // admitted up to 54,613 B; the alpha wave needs no store.)  One buffer, as vk_part with ALPHA1:
  // written before the inverse transform's barrier, read by the alpha wave between that barrier
  // and the forward transform's, which the next antenna's writes follow.  alpha_s likewise:
  // written before the forward transform's barrier, read at the combine after it, and rewritten
  // after the next antenna's inverse barrier.  Both orders rest on the two barriers alone, not on
  // which wave forms alpha.
  constexpr bool VK_LDS = MIMO_VK_LDS != 0 && ALPHA1 && sizeof(R) == 8 && wave_fft_used(F, T, true) && !CSI && T > 64;
  __shared__ R vk_thr[VK_LDS ? (T / 64 - 1) * 64 : 1];
  // The wave that forms alpha (tuning.h MIMO_ALPHA_WAVE): fixed in the fp64 wave-split instances
  // without CSI, whose wave 0 skips the inter-step twiddles; -1: wave a mod W of antenna a, as
  // every other instance has it.
  constexpr int ALPHA_WAVE = (MIMO_ALPHA_WAVE >= 0 && ALPHA1 && WAVEFFT && !CSI) ? (MIMO_ALPHA_WAVE & (W - 1)) : -1;
  // per-antenna mean |H|^2 (CSI model): dynamic LDS of A doubles (the launch sizes it), not
  // a static kMaxCsiAnt table -- the static 4 KiB cost F 4096 its second team per CU and F
  // 2048 its stage-2 twiddle rows (and with them the cot-tan FFT stages)
  extern __shared__ __align__(16) unsigned char dyn_lds[];
  R* pw_csi = reinterpret_cast<R*>(dyn_lds);
  __shared__ C symw_s[SYMW_LDS ? NSLOT * T : 1];  // [slot][thread]
  // wave-split FFT: the one-wave sub-transforms read stage 1's twiddles and (without CSI)
  // stage 2's rows r = 3, 5, 6 from LDS (team_fft.h TWL_N; -24 f64 ops per antenna at config 2)
  constexpr bool LTW1 = WAVEFFT;
  constexpr int TW1_N = [] {
    if constexpr (LTW1) return FFT::TWL_N; else return 1;
  }();
  __shared__ C tw1_s[TW1_N];
  const C* tw1 = LTW1 ? tw1_s : nullptr;

  const int t = threadIdx.x;
  const bool t0 = (t == 0);
  // the thread's sub-carriers: bins tf + T m of the FFT's frequency layout (tf = t except for
  // the split FFT, whose layout is cyclic in a permuted thread index; tf = 0 iff t = 0)
  const int tf = FFT::freq_thread(t);
  const int lane = t & 63, wid = t >> 6;
  const uint32_t trial = (uint32_t)(p.first_trial + (blockIdx.x - p0.point_start[pi]));
  const Key key{(uint32_t)p.seed, (uint32_t)(p.seed >> 32)};
  // CSI error draws: per trial with a rerolled channel (set_precoding_and_recalculate_agc
  // per trial, mp_model.py:206); with a fixed channel (CH_TABLE, reroll_chan=False) the
  // reference draws the erroneous estimate once (Link.__init__, mp_model.py:87) and keeps
  // it for every trial, so all trials share one draw (trial-independent counter).
  const uint32_t csi_trial = CH == CH_TABLE ? kFixedCsiTrial : trial;
  // ... and it belongs to the Link, not to the run: keyed by the engine's csi_seed
  const Key csi_key = CH == CH_TABLE ? Key{(uint32_t)p.csi_seed, (uint32_t)(p.csi_seed >> 32)} : key;
  // Channel counter: the trial, or (diagnostic, chan_period > 0) the trial modulo the
  // period -- every group of chan_period trials replays one sequence of Rayleigh channels,
  // as the reference's forked workers all replay the channel object's seeded generator
  // (channel.py:209-212, mp_model.py:61); bits and noise stay per trial.
  // Table instances: the channel counter is the entry of the channel bank, [entries][A][S] behind
  // chan_tab, that the trial reads.  chan_period holds the bank's size there (1: the one
  // create-time table) and the trial takes entry trial mod chan_period; 0: the bank was filled for
  // this launch, block by block (the TDL generator, tdl.hip), and the block takes its own entry.
  const uint32_t ch_trial = CH == CH_TABLE ? (p0.chan_period ? trial % p0.chan_period : (uint32_t)blockIdx.x)
                                           : (p0.chan_period ? trial % p0.chan_period : trial);
  const int S = p.n_sc, A = p.n_ant, L = p.qam_l, hb = p.half_bits;
  const R inv_sqrt_f = p.inv_sqrt_f;
  if constexpr (sizeof(R) == 8) fill_lut64<T>(&p, t);
  if constexpr (LTW1) fill_tw1<FFT, T>(tw1_s, WAVEFFT ? p.tw_wave : p.tw);
  if constexpr (sizeof(R) == 8 || LTW1) __syncthreads();

  // RX position for LoS / two-path (mp_model.py:190-201; y uses rx_loc_x, a reference quirk)
  double rx[3] = {0.0, 0.0, 0.0};
  if constexpr (CH == CH_LOS || CH == CH_TWOPATH) {
    const uint4 w = philox4x32_10(make_uint4(0u, trial, ST_LOC, 0u), key);
    const double u0 = (double)w.x * 2.3283064365386963e-10, u1 = (double)w.y * 2.3283064365386963e-10;
    rx[0] = p.rx_x0 - p.rx_var * 0.5 + p.rx_var * u0;
    rx[1] = p.rx_x0 - p.rx_var * 0.5 + p.rx_var * u1;
    rx[2] = p.rx_z;
  }

  // ---- transmitted labels and validity.  Labels are drawn twice (for the symbols before
  // the array pass, for the error counts after it) instead of being held across it.
  uint32_t valid_mask = 0;
  auto gen_labels = [&](int tt, uint32_t (&lab_out)[NSLOT]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      bool v;
      const int k = SL::k_of(s, tt, S, v);
      lab_out[s] = v ? qam_label<CHN::kUni>(key, k, trial, p.label_mask) : 0u;
    }
  };
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    bool v;
    SL::k_of(s, tf, S, v);
    valid_mask |= (v ? 1u : 0u) << s;
  }

  // (the thread id laundered per use: the table reads before and after the antenna loop
  // are redone, not kept live across it -- 8 doubles per thread that the F 8192 instance
  // spilled once per trial)
  auto frel_of = [&](int s) __attribute__((always_inline)) -> R {
    if constexpr (FREL) {
      return R(1);
    } else {
      bool v;
      const int k = SL::k_of(s, opaque(tf), S, v);
      return v ? p.f_rel[k] : R(1);
    }
  };

  // ---- pass 1: MRT norms over the (estimated) channel
  R nrm2[NSLOT];
  // CSI: the clean-run combine sum_a H conj(Hhat) / ||Hhat|| (mp_model.py:159-175 with the
  // estimate's precoder) is accumulated here, where H and Hhat are both at hand, and scaled
  // by 1 / ||Hhat|| once pass 1 has the norms -- not in the array pass, where its 16
  // accumulator VGPRs lived across both FFTs (the CSI instance spilled 53 KB per trial of
  // scratch writes, profiles/r05/pmc/pmc_traffic_2csi.json).
  C cc[CSI ? NSLOT : 1];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    nrm2[s] = R(0);
    if constexpr (CSI) cc[s] = czero<R>();
  }
  const bool clean_cc = CSI && p.incl_clean;
  // pass 1 of the Rayleigh CSI instances in polar form (below; MIMO_CSI_POLAR=0: Cartesian)
  constexpr bool CSI_POLAR = MIMO_CSI_POLAR != 0 && CSI && CH == CH_RAYLEIGH && ALIGNED && sizeof(R) == 8;
  // Perfect-CSI Rayleigh pass 1 of the fp64 wave-split instances (tuning.h): the array pass's
  // register budget does not bind here (its d, r, g, h and the FFT temporaries are not live
  // yet), so the thread id is laundered once per pass, not per antenna (P1_HOIST: the slot-to-
  // counter maps leave the loop, and thread 0's pair swap moves from the words to the finished
  // sums), and the weighted log sum runs as three sums per slot (P1_SUMS3).  One opaque copy per
  // pass: nothing is shared with the array pass's loop.
  constexpr bool P1_RAY64 = sizeof(R) == 8 && WAVEFFT && ALIGNED && CH == CH_RAYLEIGH && !CSI;
  constexpr bool P1_HOIST = MIMO_P1_HOIST != 0 && P1_RAY64;
  constexpr bool P1_SUMS3 = MIMO_P1_SUMS3 != 0 && P1_RAY64;
  constexpr bool P1_ACC = P1_HOIST || P1_SUMS3;
  R p1_acc[P1_SUMS3 ? 3 : 1][P1_ACC ? NSLOT : 1];
  int tl_p1 = tf;
  uint32_t q0_p1 = 0;
  if constexpr (P1_ACC) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s)
      for (int i = 0; i < (P1_SUMS3 ? 3 : 1); ++i) p1_acc[i][s] = R(0);
  }
  if constexpr (P1_HOIST) {
    tl_p1 = opaque(tf);
    q0_p1 = tl_p1 == 0 ? (uint32_t)((S >> 1) - 1) : (uint32_t)((S >> 2) - 1 + tl_p1);
  }
  for (int a = 0; a < (MIMO_ABL(p, ABL_PASS1) ? 1 : A); ++a) {
    MIMO_ISA_MARK("pass1");
    const int tl = P1_HOIST ? tl_p1 : opaque(tf);
    if constexpr (P1_ACC) {
      if (!MIMO_ABL(p, ABL_RNG)) {
        CHN::template power_acc<P1_SUMS3, !P1_HOIST, MIMO_P1_LN_DEG>(p, key, ch_trial, a, tl, q0_p1, p1_acc);
        continue;
      }
    }
    if constexpr (CH == CH_RAYLEIGH && !CSI) {
      if (!MIMO_ABL(p, ABL_RNG)) {
        R e2[NSLOT];
        CHN::power(p, key, ch_trial, a, tl, e2);
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) nrm2[s] += e2[s];
        continue;
      }
    }
    if constexpr ((CH == CH_LOS || CH == CH_TWOPATH) && !CSI) {
      R e2[NSLOT];
      CHN::power_closed(p, a, tl, rx, e2);
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) nrm2[s] += e2[s];
      continue;
    }
    if constexpr (CSI_POLAR) {
      // Rayleigh + CSI in polar form: with h = rho_h e^{j phi_h} (the FSPL ratio f_c / f_k in
      // rho_h), z = rho_z e^{j phi_z} and Hhat = a h + sc z,
      // |Hhat|^2 = a^2 rho_h^2 + sc^2 rho_z^2 + 2 a sc rho_h rho_z cos(phi_h - phi_z)
      // and h conj(Hhat) = a rho_h^2 + sc rho_h rho_z e^{j (phi_h - phi_z)}: one sine / cosine of
      // the angle words' difference (exact mod 2^32) and one sqrt per slot instead of two full
      // Box-Muller draws and the complex products (mp_model.py:264-282 restated).
      R rh2[NSLOT];
      uint32_t ah[NSLOT];
      const R sa = p.ant_rel[a];
      R pw = R(0);
      CHN::polar(key, ch_trial, ST_CHAN, (uint32_t)a, tl, S, bm_c<R>(sa * sa),
                 [&](int s, R r2, uint32_t w1) __attribute__((always_inline)) {
                   bool v;
                   const R fr = p.f_rel[SL::k_of(s, tl, S, v)];  // H keeps f_c / f_k with CSI (gen<true>)
                   rh2[s] = r2 * (fr * fr);
                   ah[s] = w1;
                   pw += rh2[s];
                 });
      pw = team_sum<T>(pw, red) / (R)S;
      if (t0) pw_csi[a] = pw;
      const R sc = p.csi_b * sqrt_ieee(pw), ca = p.csi_a;
      CHN::polar(csi_key, csi_trial, ST_CSI, (uint32_t)a, tl, S, bm_c<R>(R(1)),
                 [&](int s, R rz2, uint32_t wz) __attribute__((always_inline)) {
                   const R rhz = sqrt_n1(rh2[s] * rz2);  // both > 0: u1 < 1 always
                   R sn, cs;
                   sincos_lut(ah[s] - wz, sn, cs);
                   const R tz = sc * rhz;
                   nrm2[s] = fmar(ca * ca, rh2[s], fmar(sc * sc, rz2, fmar(R(2) * ca * tz, cs, nrm2[s])));
                   if (clean_cc) cc[s] = cadd(cc[s], mkc(fmar(ca, rh2[s], tz * cs), tz * sn));
                 });
      continue;
    }
    C h[NSLOT];
    CHN::template gen<FREL>(p, key, ch_trial, a, tl, rx, h);
    if constexpr (CSI) {
      // mp_model.py:264-282: Hhat = sqrt(1-eps^2) H + eps sqrt(mean_k |H|^2) z
      // (a team_sum -- two barriers -- per antenna: collecting every antenna's wave partials
      // without barriers and regenerating |H|^2 in a pass before this one measured +8 % at
      // config 2 geometry with CSI, profiles/r04/csi/: the barriers cost less than the
      // extra channel draws)
      R pw = R(0);
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) pw = fmar(h[s].x, h[s].x, fmar(h[s].y, h[s].y, pw));
      pw = team_sum<T>(pw, red) / (R)S;
      if (t0) pw_csi[a] = pw;
      C zc[NSLOT];
      CHN::normals(csi_key, csi_trial, ST_CSI, (uint32_t)a, tl, S, zc);
      const R sc = p.csi_b * sqrt_ieee(pw);
      if (clean_cc) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
          const C e = mkc(fmar(p.csi_a, h[s].x, sc * zc[s].x), fmar(p.csi_a, h[s].y, sc * zc[s].y));
          cc[s] = cadd(cc[s], cmulc(h[s], e));
          h[s] = e;
        }
      } else {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s)
          h[s] = mkc(fmar(p.csi_a, h[s].x, sc * zc[s].x), fmar(p.csi_a, h[s].y, sc * zc[s].y));
      }
    }
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) nrm2[s] = fmar(h[s].x, h[s].x, fmar(h[s].y, h[s].y, nrm2[s]));
  }
  if constexpr (P1_ACC) {
    if (!MIMO_ABL(p, ABL_RNG)) {
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        if constexpr (P1_SUMS3) nrm2[s] = ln_sum(p1_acc[0][s], p1_acc[1][s], p1_acc[2][s]);
        else nrm2[s] = p1_acc[0][s];
      }
      if constexpr (P1_HOIST) {
        // thread 0's first pair was drawn unswapped: bins S/2 and S/4 are slots 0 and Q
        constexpr int Q = SL::HALF / 2;
        const R n0 = nrm2[0], nq = nrm2[Q];
        nrm2[0] = t0 ? nq : n0;
        nrm2[Q] = t0 ? n0 : nq;
      }
    }
  }
  R inv_nrm[NSLOT];
  R etac_p = R(0);  // sum_k ||Hhat_k||^2 for the clean-run noise scaler (mp_model.py:304)
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const bool v = (valid_mask >> s) & 1u;
    inv_nrm[s] = v ? rsq_r(nrm2[s]) : R(0);
    if constexpr (CSI) cc[s] = cscale(cc[s], inv_nrm[s]);
    const R fr = frel_of(s);
    etac_p += v ? nrm2[s] * (fr * fr) : R(0);
  }
  // etac_p is used only by the clean run after the array pass: pinned here, or the compiler
  // sinks its sum into that conditional block and carries nrm2 and f_rel (16 doubles at
  // F 8192) across the antenna loop -- spilled once per trial
  asm volatile("" : "+v"(etac_p));
  if constexpr (CSI) __syncthreads();  // pw_csi visible

  C d[P];
  C r[NSLOT];
  R g[NSLOT];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    r[s] = czero<R>();
    g[s] = R(0);
  }

  // ---- array pass: precode -> IFFT -> PA -> FFT -> combine, one antenna at a time.
  // MAIN: symbols = tx labels, combine with the true channel, accumulate g (alpha_a).
  // MCNC: symbols = detected labels, combine with the estimated channel (corrector.py:198-200).
  // The symbols enter pre-weighted, symw = s / ||Hhat|| / sqrt(F) (0 on invalid slots).
  // SYMW_RE (register diet, symbols not in LDS): keep the lattice levels (qam_levels,
  // 1 VGPR per slot) and rebuild the symbol per antenna instead of holding it (4 VGPRs
  // in fp64); the opaque copies stop the compiler from hoisting it back out of the loop.
  // Register diet of the fp64 F = 8192 instance (-2.1 %; at F 2048 the |Hhat|^2 half measured
  // +0.8 %): symbols rebuilt from the labels per antenna, |Hhat|^2 recomputed after the FFT.
  // (every fp64 instance without symbols in LDS: F <= 2048 at 3 waves/SIMD, F 8192)
  constexpr bool SYMW_RE = !SYMW_LDS && sizeof(R) == 8;  // off: +13 % at F 8192
  // Precode with w = 1 / ||Hhat|| / sqrt(F) folded into the channel first (vk then sums
  // |Hhat w|^2 = vk / F): -1.1 % at F 2048 (wave-split instances); +5 % at F 4096, where
  // the 16-point team's register allocation suffers (profiles/r03/ab_o/ab_paper.json).
  // Round 6, with the cold paths out of line: at F 4096 too (not with CSI): paper -2.8 %, paper
  // CNC 0-8 -2.7 % on top of them; paper CSI +3.1 % (profiles/r06/k4096/)
  // ... and at F 8192 (not with CSI): config-5 array -1.3 %, -1.6 % with the SALU Philox rounds
  // (profiles/r06/k8192/ab_5su.json)
  // Not with CSI since round 6: the F 2048 CSI line -1.3 % without it (profiles/r06/k2048/),
  // as at F 4096 (+3.1 % with it)
  constexpr bool PRE_EW = SYMW_RE && ((WAVEFFT && (!CSI || MIMO_PRE_EW_CSI != 0)) ||
                                      (F == 4096 && !CSI && MIMO_PRE_EW_4096 != 0) ||
                                      (F == 8192 && !CSI && MIMO_PRE_EW_8192 != 0));
  // General-p Rapp out of line, and the alpha fallback by the segment table (alpha_fit.h).
  // Rounds 3-5 kept the 16-point F 4096 team's library forms inline (outlined Rapp +1.6 %,
  // r03 ab_s; with the segment table +0.8 %, profiles/r04/alpha/).  Round 6: out of line at F 4096 too -- the instance's scratch 492 -> 288 B/lane, its
  // measured traffic 54 -> 15 KB per trial, paper -1.0 %, paper CSI -1.2 % (profiles/r06/k4096/;
  // +1.6 % in round 3, before the later register cuts)
  constexpr bool COLD_OUT = sizeof(R) == 8 && (F != 4096 || MIMO_COLD_OUT_4096 != 0);
  // |Hhat|^2 for g recomputed after the FFT from the channel (fp64; off: +2.8 % at F 8192,
  // ab_diet_prefetch.json) -- except with CSI, where that would keep the 16-VGPR estimate
  // live across both FFTs next to the true channel: 8 VGPRs of |Hhat|^2 instead.
  constexpr bool E2_RE = sizeof(R) == 8 && !SYMW_LDS && (!CSI || MIMO_E2_RE_CSI != 0);
  C symw_r[SYMW_LDS || SYMW_RE ? 1 : NSLOT];
  // F 8192 (one team per CU, 256 VGPRs): the lattice levels live in LDS ([slot][thread],
  // thread-private: no barrier), not in 8 VGPRs that the allocator reloaded from scratch
  // per antenna.  (Not with CSI: its power table leaves no room.)
  constexpr bool SLAB_LDS = SYMW_RE && F >= 8192 && !CSI && NSLOT * T * 4 <= 16384;
  // In registers at F 4096 (256 VGPRs, 12 scratch reloads per antenna): two slots per word
  // (qam_levels8), -2.2 % on the paper config; at F 2048 (168 VGPRs, no reloads in the loop)
  // one word per slot, the packed form measured neutral to +0.3 % (profiles/r04/levels8/).
  constexpr bool SLAB8 = SYMW_RE && !SLAB_LDS && F == 4096 && MIMO_SLAB8_4096 != 0;
  uint32_t slab_r[SYMW_RE && !SLAB_LDS ? (SLAB8 ? NSLOT / 2 : NSLOT) : 1];
  __shared__ uint32_t slab_s[SLAB_LDS ? NSLOT * T : 1];
  // the lattice point of slot s (the word laundered: rebuilt per antenna, not hoisted)
  auto slab_point = [&](int s) __attribute__((always_inline)) -> C {
    if constexpr (SLAB_LDS) {
      uint32_t l = slab_s[s * T + t];
      asm volatile("" : "+v"(l));
      return levels_point<R>(l);
    } else if constexpr (SLAB8) {
      uint32_t w = slab_r[s >> 1];
      asm volatile("" : "+v"(w));
      return (s & 1) ? levels_point8<R, 1>(w) : levels_point8<R, 0>(w);
    } else {
      uint32_t l = slab_r[s];
      asm volatile("" : "+v"(l));
      return levels_point<R>(l);
    }
  };
  auto set_symbols = [&](const uint32_t (&lab_in)[NSLOT]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      if constexpr (SYMW_RE) {
        if constexpr (SLAB_LDS) {
          slab_s[s * T + t] = qam_levels(lab_in[s], L, hb);
        } else if constexpr (SLAB8) {
          const uint32_t v = qam_levels8(lab_in[s], L, hb);
          slab_r[s >> 1] = (s & 1) ? (slab_r[s >> 1] | (v << 16)) : v;
        } else {
          slab_r[s] = qam_levels(lab_in[s], L, hb);
        }
      } else {
        const C v = cscale(qam_point<R>(lab_in[s], L, hb), inv_nrm[s] * inv_sqrt_f);
        if constexpr (SYMW_LDS) symw_s[s * T + t] = v; else symw_r[s] = v;
      }
    }
  };
  auto symw = [&](int s) __attribute__((always_inline)) -> C {
    if constexpr (SYMW_RE) {
      R in = inv_nrm[s];
      asm volatile("" : "+v"(in));
      return cscale(slab_point(s), in * inv_sqrt_f);
    } else if constexpr (SYMW_LDS) {
      return symw_s[s * T + t];
    } else {
      return symw_r[s];
    }
  };
  // WSC: the weight w = 1 / ||Hhat|| / sqrt(F) per slot is what the antenna loops hold
  // (1 / ||Hhat|| is rederived from it after the main pass): no per-antenna multiply and no
  // laundering copy of 1 / ||Hhat||, 8 VALU per antenna: config 2 -0.2 %, MCNC -0.6 %, but the
  // CSI instance +5.3 % (its allocation again), so not with CSI (profiles/r05/ab/ab_*_wsc.json).
  constexpr bool WSC = PRE_EW && !CSI;
  // ... and for the Rayleigh channel the weight is folded into the Box-Muller radius
  // (CHN::normals_w): one multiply per draw instead of three, |h w|^2 from the radius
  constexpr bool WSC_RAY = MIMO_WSC_RAY != 0 && WSC && CH == CH_RAYLEIGH && ALIGNED;  // (fp64: no pipelined draws)
  // the draws' series cut to what their use needs in the wave-split instances only (tuning.h);
  // the team-FFT sizes keep the full series
  constexpr int BM_LN_DEG = WAVEFFT ? MIMO_BM_LN_DEG : 6;
  constexpr int BM_SIN_DEG = WAVEFFT ? MIMO_BM_SIN_DEG : 7;
  R wsc[WSC ? NSLOT : 1];
  // spectrum instances: the thread's in-band sums over the main pass (|x|^2, Re / Im of y conj(x))
  R sp_ex = R(0), sp_cre = R(0), sp_cim = R(0);
  // envelope instances: the team's histograms (cell (side, bin) of copy c at (side kEnvBins + bin)
  // SUBH + c: the copies of a bin in neighbouring banks) and the thread's sums over the main pass
  constexpr int SUBH = MIMO_ENV_SUBH;
  static_assert(SUBH >= 1 && (SUBH & (SUBH - 1)) == 0 && SUBH <= 64, "a power of two of lane residues");
  __shared__ uint32_t env_hist[ENV ? 2 * kEnvBins * SUBH : 1];
  R en_pin = R(0), en_pout = R(0), en_cre = R(0), en_cim = R(0);
  // XADDR (tuning.h; fp64 wave-split instances without CSI): the thread's LDS addresses of the two
  // transforms, packed two per word (wave_fft.h XAddr), formed here once per trial and held
  // through the main pass and the MCNC passes; the transforms launder the words, not the thread
  // id.  The receiver-phase transforms (once per iteration) keep re-deriving.
  constexpr bool XADDR =
      MIMO_XADDR != 0 && WAVEFFT && sizeof(R) == 8 && !CSI && xaddr_inst_ok(F, MODE, ALIGNED, CH);
  using XAD = typename XAddrOf<FFT, XADDR>::type;
  XAD xaddr;
  if constexpr (XADDR) xaddr.set(t, __builtin_amdgcn_readfirstlane(wid));
  auto array_pass = [&](bool main_pass, C (&acc)[NSLOT]) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) acc[s] = czero<R>();
    // Software pipeline (PIPE): antenna a+1's channel draws (one Philox call per chunk)
    // run inside antenna a's FFT exchanges, where the wave otherwise waits on LDS.
    // fp64 at F <= 4096: off (the pipelined draws' registers cost more than the exchange
    // windows hide: -1.8 % without at F 2048, profiles/r02/ab/ab64_2048.json; -2.3 % at
    // F 4096 with the wave-split FFT, scratch 140 -> 36 B/lane, profiles/r02/ab/ab4k_pipe_off.json).
    // fp64 at F 8192: -20 % without (profiles/r02/ab/ab8k_f64_team_pipe.json): fp64 never pipelines.
    constexpr bool PIPE = ALIGNED && CH == CH_RAYLEIGH && !CSI && sizeof(R) == 4;
    C hnext[PIPE ? NSLOT : 1];
    if constexpr (PIPE) {
      const R sa = p.ant_rel[0];
      if (MIMO_ABL(p, ABL_RNG)) CHN::template gen<FREL>(p, key, ch_trial, 0, tf, rx, hnext);
      else CHN::normals(key, ch_trial, ST_CHAN, 0u, tf, S, hnext, bm_c<R>(sa * sa));
    }
    for (int a = 0; a < A; ++a) {
      MIMO_ISA_MARK("array_pass");
      const int tl = opaque(tf);
      C h[NSLOT];
      R rw[WSC_RAY ? NSLOT : 1];  // WSC_RAY: |h w| per slot
      if constexpr (PIPE) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) h[s] = hnext[s];
      } else if constexpr (WSC_RAY) {
        if (MIMO_ABL(p, ABL_RNG)) {  // ablation: the synthetic channel, scaled
          CHN::template gen<FREL>(p, key, ch_trial, a, tl, rx, h);
#pragma unroll
          for (int s = 0; s < NSLOT; ++s) {
            h[s] = cscale(h[s], wsc[s]);
            rw[s] = sqrt_ieee(fmar(h[s].x, h[s].x, h[s].y * h[s].y));
          }
        } else {
          const R sa = p.ant_rel[a];
          CHN::template normals_w<BM_LN_DEG, BM_SIN_DEG>(key, ch_trial, ST_CHAN, (uint32_t)a, tl, S, bm_c<R>(sa * sa), wsc,
                                                         h, rw);
        }
      } else {
        CHN::template gen<FREL>(p, key, ch_trial, a, tl, rx, h);
        if constexpr (WSC) {
#pragma unroll
          for (int s = 0; s < NSLOT; ++s) h[s] = cscale(h[s], wsc[s]);
        }
      }
      const int an = a + 1 < A ? a + 1 : a;
      const R san = PIPE ? p.ant_rel[an] : R(0);
      // Window w of NW = 2 XCHG exchange windows (IFFT then FFT) draws chunks
      // [w NC / NW, (w + 1) NC / NW) of antenna a+1.  After the last antenna the draws are
      // redone for it and unused: a uniform branch around them measured 2.7 % slower (it
      // splits the exchange windows' basic blocks; profiles/r02/ab/ab32_lastant.json).
      // Ablation ABL_RNG: antenna a+1's synthetic channel, in window 0.
      auto hfill = [&](int w) __attribute__((always_inline)) {
        if constexpr (PIPE) {
          constexpr int NC = CHN::kChunks, NW = 2 * FFT::XCHG;
          if (MIMO_ABL(p, ABL_RNG)) {
            if (w == 0) CHN::template gen<FREL>(p, key, ch_trial, an, tl, rx, hnext);
          } else {
#pragma unroll
            for (int c = 0; c < NC; ++c)
              if (c >= w * NC / NW && c < (w + 1) * NC / NW)
                CHN::normals_chunk(c, key, ch_trial, ST_CHAN, (uint32_t)an, tl, S, hnext, bm_c<R>(san * san));
          }
        }
      };
      auto hfill_ifft = [&](int w) __attribute__((always_inline)) { hfill(w); };
      auto hfill_fft = [&](int w) __attribute__((always_inline)) { hfill(FFT::XCHG + w); };
      C he[CSI ? NSLOT : 1];
      if constexpr (CSI) {
        // (regenerated, not staged: the error term written to HBM in pass 1 and read back
        // here measured +11 %, profiles/r05/ab/ab_2csi_stage_r05e.json)
        C zc[NSLOT];
        CHN::normals(csi_key, csi_trial, ST_CSI, (uint32_t)a, tl, S, zc);
        const R sc = p.csi_b * sqrt_ieee(pw_csi[a]);
#pragma unroll
        for (int s = 0; s < NSLOT; ++s)
          he[s] = mkc(fmar(p.csi_a, h[s].x, sc * zc[s].x), fmar(p.csi_a, h[s].y, sc * zc[s].y));
      }
      auto hest = [&](int s) __attribute__((always_inline)) -> C {
        if constexpr (CSI) return he[s]; else return h[s];
      };
      // vk_part / alpha_s buffer: with ALPHA1 one (the designated wave reads vk_part(a) and
      // every wave alpha(a) before the next antenna's IFFT barrier, which the next writes
      // follow): compile-time LDS addresses; otherwise every wave reads vk_part(a) after the
      // forward FFT, racing the next antenna's writes -- two buffers
      const int vkb = ALPHA1 ? 0 : (a & 1);
      C x[NSLOT];
      R e2[NSLOT];  // |Hhat|^2, kept for g after the FFT
      R vk = R(0);
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        const C e = hest(s);
        if constexpr (PRE_EW) {
          // the lattice point times conj(Hhat w), w = 1 / ||Hhat|| / sqrt(F): vk accumulates
          // |Hhat w|^2 = |Hhat|^2 / ||Hhat||^2 / F directly (11 f64 ops per slot, not 13;
          // vk_scale restores the factor F)
          C ew;
          if constexpr (WSC) {
            ew = e;  // the loops carry h w already
          } else {
            R in = inv_nrm[s];
            asm volatile("" : "+v"(in));
            ew = cscale(e, in * inv_sqrt_f);
          }
          x[s] = cmulc(slab_point(s), ew);
          if constexpr (WSC_RAY) vk = fmar(rw[s], rw[s], vk);
          else vk = fmar(ew.x, ew.x, fmar(ew.y, ew.y, vk));
          if constexpr (!E2_RE) e2[s] = fmar(e.x, e.x, e.y * e.y);
        } else {
          x[s] = cmulc(symw(s), e);  // s conj(Hhat) / ||Hhat|| / sqrt(F); 0 off band (symw = 0)
          e2[s] = fmar(e.x, e.x, e.y * e.y);
          vk = fmar(e2[s], inv_nrm[s] * inv_nrm[s], vk);  // inv_nrm = 0 off band
        }
        if constexpr (SPEC) {
          if (main_pass) sp_ex = fmar(x[s].x, x[s].x, fmar(x[s].y, x[s].y, sp_ex));
        }
      }
      if (main_pass) {
        if constexpr (VK_LDS) {
          // (read after the IFFT's first barrier)
          if constexpr (ALPHA_WAVE >= 0) {
            if (wid != ALPHA_WAVE) vk_thr[(wid - (wid > ALPHA_WAVE ? 1 : 0)) * 64 + lane] = vk;
          } else {
            const int aw = a & (W - 1);
            if (wid != aw) vk_thr[((wid - aw - 1) & (W - 1)) * 64 + lane] = vk;
          }
        } else {
          vk = wave_sum_lane63(vk);
          if (lane == 63) vk_part[vkb][wid] = vk;  // read after the IFFT's first barrier
        }
      }
      SL::scatter(d, x, t0);
      if constexpr (BEAM) {
        if (main_pass) {
          // X_a / sqrt(F) as scattered (0 off band): the buffer's second half, bin tl + T m
          double2* cell = reinterpret_cast<double2*>(std::get<kModeOut>(ma)) +
                          ((size_t)gridDim.x * (size_t)A + (size_t)blockIdx.x * (size_t)A + (size_t)a) * (size_t)F + tl;
#pragma unroll
          for (int m = 0; m < P; ++m) cell[T * m] = make_double2((double)d[m].x, (double)d[m].y);
        }
      }
      // the FFTs take the thread id already laundered for this antenna (tl) where it is the
      // physical one: their own opaque copy of it then costs no register move in run_second
      const int tfft = SPLITFFT ? t : tl;
      if (!MIMO_ABL(p, ABL_FFT)) {
        if constexpr (XADDR)
          FFT::template run<+1, 0, SL::zero_mask()>(d, lds, p.tw_wave, xaddr, tfft, MIMO_ABL(p, ABL_XCHG), hfill_ifft, tw1);
        else
          FFT::template run<+1, 0, SL::zero_mask()>(d, lds, WAVEFFT ? p.tw_wave : p.tw, tfft, MIMO_ABL(p, ABL_XCHG),
                                                    hfill_ifft, tw1);
      }
      C xin[ENV ? P : 1];  // envelope instances: the PA input, held across pa_block
      if constexpr (ENV) {
        if (main_pass) {
#pragma unroll
          for (int m = 0; m < P; ++m) {
            xin[m] = d[m];
            const R pw = fmar(d[m].x, d[m].x, d[m].y * d[m].y);
            en_pin += pw;
#ifndef MIMO_DIAG_ENV_NOHIST  // cost breakdowns only: the sums and the held x without the histograms
            atomicAdd(&env_hist[env_bin((double)pw, std::get<kModeScale>(ma)) * SUBH + (lane & (SUBH - 1))], 1u);
#endif
          }
        }
      }
      if (!MIMO_ABL(p, ABL_PA)) pa_block<COLD_OUT>(p.pa_kind, d, p.sat_tx, p.sqrt_sat_tx, p.inv_sat_tx, p.rapp_p, p.toi_tx);
      if constexpr (ENV) {
        if (main_pass) {
#pragma unroll
          for (int m = 0; m < P; ++m) {
            const R pw = fmar(d[m].x, d[m].x, d[m].y * d[m].y);
            en_pout += pw;
#ifndef MIMO_DIAG_ENV_NOHIST
            atomicAdd(&env_hist[(kEnvBins + env_bin((double)pw, std::get<kModeScale>(ma))) * SUBH + (lane & (SUBH - 1))], 1u);
#endif
            en_cre = fmar(d[m].x, xin[m].x, fmar(d[m].y, xin[m].y, en_cre));
            en_cim = fmar(d[m].y, xin[m].x, fmar(-d[m].x, xin[m].y, en_cim));
          }
        }
      }
      // alpha_a (Bussgang gain of antenna a's PA from its precoding power, main pass only)
      auto alpha_of_vk = [&]() __attribute__((always_inline)) -> R {
        R vks;
        if constexpr (VK_LDS) {
          // the alpha wave: its own partials and the other waves', region by region, then the
          // one tree; lane 63's sum to every lane, so that the branches below stay uniform
          if constexpr (ALPHA_WAVE >= 0) {  // in wave order, the alpha wave's own in its place
            vks = ALPHA_WAVE == 0 ? vk : vk_thr[lane];
#pragma unroll
            for (int i = 1; i < W; ++i)
              vks += i == ALPHA_WAVE ? vk : vk_thr[(i - (i > ALPHA_WAVE ? 1 : 0)) * 64 + lane];
          } else {
            vks = vk;
#pragma unroll
            for (int i = 0; i < W - 1; ++i) vks += vk_thr[i * 64 + lane];
          }
          const uint64_t u = __builtin_bit_cast(uint64_t, (double)wave_sum_lane63(vks));
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, 63);
          const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), 63);
          vks = (R)__builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
        } else {
          vks = vk_part[vkb][0];
#pragma unroll
          for (int i = 1; i < W; ++i) vks += vk_part[vkb][i];
        }
        const R x = fmar(vks, PRE_EW ? p.inv_vk0_f : p.inv_vk0, -R(1));
        // Polynomial alpha: -7 % at F = 2048, but +3 % at F = 8192 (SGPR pressure of the
        // 8 waves/team instance, tools/ab_libs.py), so only up to F = 4096.
        if (sizeof(R) == 4 && F <= 4096 && absr(x) <= p.alpha_xlim) {
          R acc = p.apoly[8];
#pragma unroll
          for (int i = 7; i >= 0; --i) acc = fmar(acc, x, p.apoly[i]);
          return acc;
        } else if (sizeof(R) == 8 && absr(x) <= p.alpha_xlim) {
          // Horner, 18 FMAs with the coefficients as SGPR operands instead of the library
          // exp + erfc.  (Plain fma() compiles to v_fmac_f64 and copies every coefficient
          // into the accumulator's VGPRs first, 2 v_mov per step: +0.7 % at F 2048, +0.9 %
          // at F 4096, profiles/r03/ab_o.)
          double acc = p.amono64[18];
#pragma unroll
          for (int k = 17; k >= 0; --k) {
            const double ck = p.amono64[k];
            asm("v_fma_f64 %0, %1, %2, %3" : "=v"(acc) : "v"(acc), "v"((double)x), "s"(ck));
          }
          return (R)acc;
        } else {
          // (the register-diet pass sums vk / F: vks F is the precoding power)
          const R g2 = p.alpha_c / (PRE_EW ? vks * (R)F : vks);
          // fp64: the segment table (alpha_fit.h, appended to the Box-Muller tables in HBM)
          if constexpr (COLD_OUT) return alpha_seg(g2, reinterpret_cast<const double*>(p.lut + kLut64));
          else return alpha_of_gamma2(g2);
        }
      };
      // ALPHA1: one wave per antenna (ALPHA_WAVE, else a mod W) forms it from the vk partials
      // (visible since the IFFT's first barrier) and hands it over in LDS; the forward FFT's
      // cross-wave barrier orders the hand-off (alpha_s double-buffered like vk_part).  The other
      // waves skip the partial sum and the 18-FMA polynomial.
      if constexpr (ALPHA1) {
        // (ablation builds without the transforms' barriers: order the vk_part hand-off)
        if (MIMO_ABL(p, ABL_FFT) || MIMO_ABL(p, ABL_XCHG)) __syncthreads();
        if (main_pass && wid == (ALPHA_WAVE >= 0 ? ALPHA_WAVE : (a & (W - 1)))) {
          const R al = alpha_of_vk();
          if (lane == 0) alpha_s[vkb] = al;
        }
      }
      if (!MIMO_ABL(p, ABL_FFT)) {
        if constexpr (XADDR)
          FFT::template run_second<-1>(d, lds, p.tw_wave, xaddr, tfft, MIMO_ABL(p, ABL_XCHG), hfill_fft, tw1);
        else
          FFT::template run_second<-1>(d, lds, WAVEFFT ? p.tw_wave : p.tw, tfft, MIMO_ABL(p, ABL_XCHG), hfill_fft, tw1);
      }
      if constexpr (PIPE) {
        if (MIMO_ABL(p, ABL_FFT)) {  // no transforms ran, so no exchange windows (ABL_XCHG keeps them)
#pragma unroll
          for (int w = 0; w < 2 * FFT::XCHG; ++w) hfill(w);
        }
      }
      // keep the vk_part / alpha_s hand-offs ordered when the ablations drop the barriers
      if (MIMO_ABL(p, ABL_FFT) || (ALPHA1 && MIMO_ABL(p, ABL_XCHG))) __syncthreads();
      if constexpr (BEAM) {
        if (main_pass) {
          // Y_a sqrt(F): the thread's P bins of the chain output, bin tl + T m
          double2* cell =
              reinterpret_cast<double2*>(std::get<kModeOut>(ma)) + ((size_t)blockIdx.x * (size_t)A + (size_t)a) * (size_t)F + tl;
#pragma unroll
          for (int m = 0; m < P; ++m) cell[T * m] = make_double2((double)d[m].x, (double)d[m].y);
        }
      }
      if constexpr (SPEC) {
        if (main_pass) {
          // psd: |d|^2 / F (ortho) into the thread's cells, bin tl + T m; 1 / F is a power of two
          double* cell = std::get<kModeOut>(ma) + (size_t)blockIdx.x * (size_t)(F + kSpecFixed) + tl;
          R pw[P];
#pragma unroll
          for (int m = 0; m < P; ++m) pw[m] = fmar(d[m].x, d[m].x, d[m].y * d[m].y) * R(1.0 / F);
          if (a == 0) {
#pragma unroll
            for (int m = 0; m < P; ++m) cell[T * m] = (double)pw[m];
          } else {
            double old[P];
#pragma unroll
            for (int m = 0; m < P; ++m) old[m] = cell[T * m];
#pragma unroll
            for (int m = 0; m < P; ++m) cell[T * m] = old[m] + (double)pw[m];
          }
          // C: the precoder input x rebuilt from the (estimated) channel as the slot loop above
          // formed it (not held across the transforms); x = 0 off band
#pragma unroll
          for (int s = 0; s < NSLOT; ++s) {
            const C e = hest(s);
            C xs;
            if constexpr (PRE_EW) {
              C ew;
              if constexpr (WSC) {
                ew = e;
              } else {
                R in = inv_nrm[s];
                asm volatile("" : "+v"(in));
                ew = cscale(e, in * inv_sqrt_f);
              }
              xs = cmulc(slab_point(s), ew);
            } else {
              xs = cmulc(symw(s), e);
            }
            const C y = SL::gather(d, s, t0);
            sp_cre = fmar(y.x, xs.x, fmar(y.y, xs.y, sp_cre));
            sp_cim = fmar(y.y, xs.x, fmar(-y.x, xs.y, sp_cim));
          }
        }
      }
      R alpha_a = R(0);
      if (main_pass) alpha_a = ALPHA1 ? alpha_s[vkb] : alpha_of_vk();
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        const C y = SL::gather(d, s, t0);
        if (main_pass) {
          acc[s] = cmac(acc[s], h[s], y);
          if constexpr (E2_RE) {
            C e = hest(s);
            asm volatile("" : "+v"(e.x), "+v"(e.y));
            g[s] = fmar(alpha_a, fmar(e.x, e.x, e.y * e.y), g[s]);
          } else {
            g[s] = fmar(alpha_a, e2[s], g[s]);  // sum_a alpha_a |Hhat|^2; x 1/||Hhat|| after the pass
          }
        } else {
          acc[s] = cmac(acc[s], hest(s), y);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      // WSC: sum_a (h w) y = w sum_a h y
      if constexpr (WSC) acc[s] = cscale(acc[s], wsc[s] > R(0) ? inv_sqrt_f / wsc[s] : R(0));
      else acc[s] = cscale(acc[s], inv_sqrt_f);
    }
  };

  {
    uint32_t lab0[NSLOT];
    gen_labels(tf, lab0);
    set_symbols(lab0);
  }
  if constexpr (WSC) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) wsc[s] = inv_nrm[s] * inv_sqrt_f;
  }
  if constexpr (ENV) {
    for (int i = t; i < 2 * kEnvBins * SUBH; i += T) env_hist[i] = 0u;
    __syncthreads();
  }
  array_pass(true, r);
  if constexpr (ENV) {
    // the fixed sums in team_sum's order; the barrier puts every wave's ds_adds ahead of the reads
    const R pin = team_sum<T>(en_pin, red), pout = team_sum<T>(en_pout, red);
    const R cre = team_sum<T>(en_cre, red), cim = team_sum<T>(en_cim, red);
    __syncthreads();
    double* row = std::get<kModeOut>(ma) + (size_t)blockIdx.x * (size_t)(2 * kEnvBins + kEnvFixed);
    for (int i = t; i < 2 * kEnvBins; i += T) {
      uint32_t n = 0;
#pragma unroll
      for (int c = 0; c < SUBH; ++c) n += env_hist[i * SUBH + c];
      row[i] = (double)n;
    }
    if (t0) {
      row[2 * kEnvBins] = (double)pin;
      row[2 * kEnvBins + 1] = (double)pout;
      row[2 * kEnvBins + 2] = (double)cre;
      row[2 * kEnvBins + 3] = (double)cim;
    }
  }
  if constexpr (SPEC) {
    // Ex = F sum |x|^2 (x carries 1 / sqrt(F)); Y conj(X) = (d / sqrt(F)) conj(x sqrt(F)) = d conj(x)
    const R ex = team_sum<T>(sp_ex, red), cre = team_sum<T>(sp_cre, red), cim = team_sum<T>(sp_cim, red);
    if (t0) {
      double* fixed = std::get<kModeOut>(ma) + (size_t)blockIdx.x * (size_t)(F + kSpecFixed) + F;
      fixed[0] = (double)(ex * (R)F);
      fixed[1] = (double)cre;
      fixed[2] = (double)cim;
    }
  }
  if constexpr (WSC) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) inv_nrm[s] = wsc[s] / inv_sqrt_f;
  }
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    // WSC: g accumulated alpha |h w|^2 = w^2 alpha |h|^2, and inv_nrm / w^2 = 1 / (w / sqrt(F))
    if constexpr (WSC) g[s] = wsc[s] > R(0) ? g[s] / (wsc[s] * inv_sqrt_f) : R(0);
    else g[s] *= inv_nrm[s];
  }
  uint32_t lab[NSLOT];
  gen_labels(opaque(tf), lab);

  // ---- AWGN + AGC (noise.py:56-83 on all bins; only in-band bins matter)
  C zn[NSLOT];
  CHN::normals(key, trial, ST_NOISE, 0u, tf, S, zn);
  R eta_p = R(0);
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const R gs = g[s] * frel_of(s);
    eta_p = ((valid_mask >> s) & 1u) ? fmar(gs, gs, eta_p) : eta_p;
  }
  const R eta = team_sum<T>(eta_p, red) / (R)S;
  uint32_t* out = p0.counts + (size_t)blockIdx.x * p0.n_idx;

  auto record = [&](int idx, uint32_t errs) __attribute__((always_inline)) {
    const R tot = team_sum<T>((R)errs, red);
    if (t0) out[idx] = (uint32_t)(tot + R(0.5));
  };
  // measure instances: column `col` of the trial's row = the team's sum of v (team_sum's fixed order)
  auto measure = [&](int col, R v) __attribute__((always_inline)) {
    if constexpr (MEAS) {
      const R tot = team_sum<T>(v, red);
      if (t0) std::get<kModeOut>(ma)[(size_t)blockIdx.x * (size_t)(kMeasFixed + p0.n_idx) + col] = (double)tot;
    }
  };
  // soft instances: the team's reliability histogram of the counter index being recorded.  Zeroed
  // here; every flush leaves it zeroed for the next index.
  __shared__ uint32_t soft_hist[SOFT ? kSoftBins : 1];
  if constexpr (SOFT) {
    for (int i = t; i < kSoftBins; i += T) soft_hist[i] = 0u;
    __syncthreads();
  }
  // the 2 hb reliabilities of slot s, whose slicer input is v, into the histogram (valid slots only)
  auto soft_add = [&](int s, C v) __attribute__((always_inline)) {
    if constexpr (SOFT) {
      if ((valid_mask >> s) & 1u) {
        const uint32_t li = lab[s] >> hb, lq = lab[s] & ((1u << hb) - 1u);
#ifndef MIMO_DIAG_SOFT_NOHIST  // cost breakdowns only: the metric without the LDS adds
        soft_axis((double)v.x, L, hb, [&](int j, double lam) {
          atomicAdd(&soft_hist[soft_bin(lam, (li >> j) & 1u, std::get<kModeScale>(ma))], 1u);
        });
        soft_axis((double)v.y, L, hb, [&](int j, double lam) {
          atomicAdd(&soft_hist[soft_bin(lam, (lq >> j) & 1u, std::get<kModeScale>(ma))], 1u);
        });
#else
        double keep = 0.0;
        soft_axis((double)v.x, L, hb, [&](int j, double lam) { keep += (double)soft_bin(lam, (li >> j) & 1u, std::get<kModeScale>(ma)); });
        soft_axis((double)v.y, L, hb, [&](int j, double lam) { keep += (double)soft_bin(lam, (lq >> j) & 1u, std::get<kModeScale>(ma)); });
        if (keep < 0.0) atomicAdd(&soft_hist[0], 1u);  // never taken: keeps the metric alive
#endif
      }
    }
  };
  // after `record`: the histogram of counter index idx to the trial's row, and zeroed for the next.
  // The first barrier puts every wave's ds_adds ahead of the reads, the second the zeroes ahead of
  // the next index's adds; a thread zeroes the cells it read.
  auto soft_flush = [&](int idx) __attribute__((always_inline)) {
    if constexpr (SOFT) {
      __syncthreads();
      double* row = std::get<kModeOut>(ma) + ((size_t)blockIdx.x * (size_t)p0.n_idx + (size_t)idx) * (size_t)kSoftBins;
      for (int i = t; i < kSoftBins; i += T) {
        row[i] = (double)soft_hist[i];
        soft_hist[i] = 0u;
      }
      __syncthreads();
    }
  };
  // coded instances: the 2 hb channel values of slot s, whose slicer input is v, to the stream of
  // counter index idx (valid slots only; only where the index is recorded)
  auto coded_put = [&](int idx, int s, C v) __attribute__((always_inline)) {
    if constexpr (CODED) {
      bool ok;
      const int k = SL::k_of(s, opaque(tf), S, ok);
      if (ok) {
        const uint32_t li = lab[s] >> hb, lq = lab[s] & ((1u << hb) - 1u);
        int8_t* o = std::get<kModeOut>(ma) + ((size_t)blockIdx.x * (size_t)p0.n_idx + (size_t)idx) * ((size_t)S * (size_t)(2 * hb)) + k;
        soft_axis((double)v.x, L, hb, [&](int j, double lam) {
          o[(size_t)(hb - 1 - j) * (size_t)S] = (int8_t)coded_value(lam, (li >> j) & 1u, std::get<kModeScale>(ma));
        });
        soft_axis((double)v.y, L, hb, [&](int j, double lam) {
          o[(size_t)(2 * hb - 1 - j) * (size_t)S] = (int8_t)coded_value(lam, (lq >> j) & 1u, std::get<kModeScale>(ma));
        });
      }
    }
  };
  // |a - b|^2 on a valid slot, 0 off band
  auto err2 = [&](int s, C a, C b) __attribute__((always_inline)) -> R {
    const C e = csub(a, b);
    return ((valid_mask >> s) & 1u) ? fmar(e.x, e.x, e.y * e.y) : R(0);
  };

  if (p.incl_clean) {
    // clean run (mp_model.py:159-175): no PA, AGC / noise from sum_a Hhat P = ||Hhat||
    const R etac = team_sum<T>(etac_p, red) / (R)S;
    const R sig_c = sqrt_ieee(p.es_over_snr * etac);
    uint32_t errs = 0;
    R ee = R(0);
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const C sym = qam_point<R>(lab[s], L, hb);
      C rc;
      if constexpr (CSI) rc = cmul(cc[s], sym); else rc = cscale(sym, inv_nrm[s] > R(0) ? R(1) / inv_nrm[s] : R(0));
      const R ig = inv_nrm[s];  // 1 / ||Hhat||  (/ f_rel when factored)
      const R sn = sig_c / frel_of(s);
      const C zc = mkc((rc.x + sn * zn[s].x) * ig, (rc.y + sn * zn[s].y) * ig);
      const uint32_t lh = slice(zc, L, hb);
      errs += ((valid_mask >> s) & 1u) ? __popc(lh ^ lab[s]) : 0u;
      if constexpr (MEAS) ee += err2(s, zc, sym);
      soft_add(s, zc);
      coded_put(0, s, zc);
    }
    measure(kMeasFixed, ee);
    record(0, errs);
    soft_flush(0);
  }

  const R sig = sqrt_ieee(p.es_over_snr * eta);
  C z[NSLOT];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const R ig = ((valid_mask >> s) & 1u) ? R(1) / g[s] : R(0);
    const R sn = sig / frel_of(s);
    z[s] = mkc((r[s].x + sn * zn[s].x) * ig, (r[s].y + sn * zn[s].y) * ig);
    // turbo instances: z of every valid slot to the launch's buffer, sub-carrier order
    if constexpr (TURBO) {
      bool ok;
      const int k = SL::k_of(s, opaque(tf), S, ok);
      if (ok) std::get<kModeOut>(ma)[(size_t)blockIdx.x * (size_t)S + (size_t)k] = z[s];
    }
  }
  if constexpr (MEAS) {
    // the noiseless AGC'd value z0 = r / g against the transmitted point: Es, Ez0, C = sum z0 conj(s), Ed0
    R es = R(0), ez0 = R(0), cre = R(0), cim = R(0), ed0 = R(0);
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const bool v = (valid_mask >> s) & 1u;
      const C sym = qam_point<R>(lab[s], L, hb);
      const C z0 = cscale(r[s], v ? R(1) / g[s] : R(0));
      es += v ? fmar(sym.x, sym.x, sym.y * sym.y) : R(0);
      ez0 += v ? fmar(z0.x, z0.x, z0.y * z0.y) : R(0);
      cre += v ? fmar(z0.x, sym.x, z0.y * sym.y) : R(0);
      cim += v ? fmar(z0.y, sym.x, -(z0.x * sym.y)) : R(0);
      ed0 += err2(s, z0, sym);
    }
    measure(0, es);
    measure(1, ez0);
    measure(2, cre);
    measure(3, cim);
    measure(4, ed0);
  }

  // ---- CNC / MCNC receiver.  One loop per receiver kind (a uniform branch outside the
  // loops): the CNC loop then holds neither the MCNC-only state (g, 1/||Hhat||, the
  // symbols' LDS) nor its code, so it runs without the register spills a shared loop had.
  C dist[NSLOT];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) dist[s] = czero<R>();
  int idx = p.incl_clean;
  // slice z - dist, count and record iteration `it`; false once the last one is recorded
  auto detect = [&](int it, uint32_t (&lh)[NSLOT]) __attribute__((always_inline)) -> bool {
    uint32_t errs = 0;
    R ee = R(0);
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      lh[s] = slice(csub(z[s], dist[s]), L, hb);
      errs += ((valid_mask >> s) & 1u) ? __popc(lh[s] ^ lab[s]) : 0u;
      if constexpr (MEAS) ee += err2(s, csub(z[s], dist[s]), qam_point<R>(lab[s], L, hb));
    }
    if ((p.rec_mask >> it) & 1u) {
      if constexpr (SOFT) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) soft_add(s, csub(z[s], dist[s]));
      }
      if constexpr (CODED) {
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) coded_put(idx, s, csub(z[s], dist[s]));
      }
      measure(kMeasFixed + idx, ee);
      record(idx++, errs);
      soft_flush(idx - 1);
    }
    return it < p.max_iter;
  };
  if (p.receiver == RX_CNC) {
    for (int it = 0;; ++it) {
      uint32_t lh[NSLOT];
      if (!detect(it, lh)) break;
      // corrector.py:84-110: single-antenna re-synthesis of the clipping distortion
      C x[NSLOT];
#pragma unroll
      for (int s = 0; s < NSLOT; ++s)
        x[s] = ((valid_mask >> s) & 1u) ? cscale(qam_point<R>(lh[s], L, hb), inv_sqrt_f) : czero<R>();
      SL::scatter(d, x, t0);
      FFT::template run<+1, 0, SL::zero_mask()>(d, lds, WAVEFFT ? p.tw_wave : p.tw, t, false,
                                                typename FFT::NoFill{}, tw1);
      pa_block<COLD_OUT>(p.cnc_pa_kind, d, p.sat_cnc, p.sqrt_sat_cnc, p.inv_sat_cnc, p.rapp_p, p.toi_cnc);
      FFT::template run_second<-1>(d, lds, WAVEFFT ? p.tw_wave : p.tw, t, false, typename FFT::NoFill{}, tw1);
      const R sc = inv_sqrt_f * p.inv_alpha_cnc;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        const C y = SL::gather(d, s, t0);
        dist[s] = ((valid_mask >> s) & 1u) ? csub(cscale(y, sc), qam_point<R>(lh[s], L, hb)) : czero<R>();
      }
    }
  } else {
    // corrector.py:165-207: re-transmit the detected symbols through the whole array
    for (int it = 0;; ++it) {
      uint32_t lh[NSLOT];
      if (!detect(it, lh)) break;
      C est[NSLOT];
      set_symbols(lh);
      array_pass(false, est);
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        const R ig = ((valid_mask >> s) & 1u) ? R(1) / g[s] : R(0);
        dist[s] = ((valid_mask >> s) & 1u) ? csub(cscale(est[s], ig), qam_point<R>(lh[s], L, hb))
                                           : czero<R>();
      }
    }
  }
}

}  // namespace mimo
