// The host / device contract of the fused trial kernel (trial_kernel.h): what the host code
// (engine.hip, host_tables.h, trial_launch.h) may rely on without seeing the kernel -- the kinds, the
// run modes and their kernel arguments, the row layouts of the row modes, and TrialParams.
// No device function and no tuning switch lives here.
#pragma once
#include <stdint.h>

#include <tuple>
#include <type_traits>

#include "real.h"

namespace mimo {

enum PaKind : int { PA_NONE = 0, PA_SOFTLIM = 1, PA_RAPP = 2, PA_TOI = 3 };
enum ChanKind : int { CH_RAYLEIGH = 1, CH_LOS = 2, CH_TWOPATH = 3, CH_TABLE = 4 };
enum RxKind : int { RX_CNC = 1, RX_MCNC = 2 };

// The run mode of an instance: trial_kernel's first template argument (macros, since the Makefile
// hands one to each trial_inst.hip object as -DINST_MODE=<mode>).  The seven row modes are float64 only.
#define MIMO_MODE_PLAIN 0  // the counts alone
#define MIMO_MODE_MEAS 1
#define MIMO_MODE_SPEC 2
#define MIMO_MODE_BEAM 3
#define MIMO_MODE_ENV 4
#define MIMO_MODE_SOFT 5
#define MIMO_MODE_CODED 6
#define MIMO_MODE_TURBO 7

// What a mode's kernel takes behind TrialParams, each argument with its true type: the buffer its
// instances fill (kModeOut; the sections below have the layouts) and the mode's scale (kModeScale).
// (A tuple, since the kernel takes its members as arguments of their own: one struct of the two
// would be passed by reference and read at the kernel's entry, and an empty stand-in would move the
// implicit arguments.)  TrialParams itself stays the stride of the per-point table, and its layout is
// tuned (see csi_seed).
template <int MODE>
using ModeArgs = std::conditional_t<
    MODE == MIMO_MODE_PLAIN, std::tuple<>,                                                // nothing
    std::conditional_t<MODE == MIMO_MODE_CODED, std::tuple<int8_t*, double>,              // channel values, 32 / rho_max
                       std::conditional_t<MODE == MIMO_MODE_ENV || MODE == MIMO_MODE_SOFT,
                                          std::tuple<double*, double>,                    // rows, the bin scale
                                          std::conditional_t<MODE == MIMO_MODE_TURBO, std::tuple<double2*>,  // the received vectors
                                                             std::tuple<double*>>>>>;     // measure, spectrum: rows; beam: cells
constexpr int kModeOut = 0, kModeScale = 1;

// Measure instances (MIMO_MODE_MEAS): the same trial, the same
// counts, and per trial a row of kMeasFixed + n_idx power sums over the valid in-band slots
// (include/mimo_engine.h mimo_engine_measure_points: Es, Ez0, Re C, Im C, Ed0, then Ee_i per
// counter index).  The row pointer is an argument of those instances alone (ModeArgs), and the plain
// instances compile to the code they had (profiles/r08/measure/isa_diff.txt).
constexpr int kMeasFixed = 5;  // MIMO_MEAS_FIXED

// Spectrum instances (MIMO_MODE_SPEC): the same trial, the same
// counts, and per trial a row of F + kSpecFixed doubles from the main array pass alone
// (include/mimo_engine.h mimo_engine_spectrum_points): psd[k] = sum_a |Y_a[k]|^2 for every FFT
// bin k (numpy.fft order, ortho transform pair), then Ex = sum_a sum_band |X_a|^2 and Re / Im of
// C = sum_a sum_band Y_a conj(X_a).  After the forward transform register m of frequency thread
// tf holds bin tf + T m in every FFT kind (plain and wave-split teams: tf = t; the F 8192 split
// FFT: tf = 2 vt + g, so bin 2 (vt + 256 m) + g -- csrc/probe.hip writes its outputs by the same
// statement).  psd accumulator: a read-modify-write of the thread's own P cells of the trial's
// row once per antenna (antenna 0 stores), in antenna order, no atomics and no synchronisation;
// the rows of the teams in flight stay L2-resident.  (One form for all sizes: from F 256 up the
// instances sit at their register cap with scratch already -- 168 VGPRs up to F 2048, 256 from
// F 4096 -- so P more f64 registers would spill to the same memory.)  As for the measure
// instances the row pointer is an extra argument of those instances alone.
constexpr int kSpecFixed = 3;  // MIMO_SPEC_FIXED

// Beam instances (MIMO_MODE_BEAM): the same trial, the same
// counts, and the main array pass hands every antenna's chain to the beamforming kernel
// (beam.hip; include/mimo_engine.h mimo_engine_beam_points) through a per-launch buffer of
// complex128 cells: [grid.x][A][F] of the chain output's registers d (Y_a = d / sqrt(F)), then
// [grid.x][A][F] of the precoder input where Slots::scatter placed it (X_a = d sqrt(F), 0 off
// band).  Register m of frequency thread tf is bin tf + T m before the inverse and after the
// forward transform (the spectrum instances' statement).  Plain 16-byte stores, every cell
// written once per launch; the buffer pointer is an extra argument of those instances alone.

// Envelope instances (MIMO_MODE_ENV): the same trial, the same
// counts, and per trial a row of 2 kEnvBins + kEnvFixed doubles from the main array pass alone
// (include/mimo_engine.h mimo_engine_envelope_points): the histograms of |x_a[n]|^2 and |y_a[n]|^2
// over every antenna's F time samples -- d between the inverse transform and pa_block is x_a (the
// precoder input carries 1 / sqrt(F), so the unnormalised inverse is the ortho one), d after it
// y_a -- then Pin = sum |x|^2, Pout = sum |y|^2 and Re / Im of sum y conj(x).  Bins (env_bin):
// eight linear sub-bins per octave read off the bits of pw scale.  Counters: uint32 in a per-team
// LDS histogram, zeroed before the pass, one ds_add_u32 per sample and side, stored to the row as
// doubles once after the pass (plain stores, no global atomics).  MIMO_ENV_SUBH (tuning.h) copies of
// the histogram, one per lane residue, spread the lanes that meet in the few bins around the mean.
// x is held across pa_block in a copy of d (4 P VGPRs; the instances up to F 2048 are therefore
// built for 2 waves / SIMD, tuning.h MIMO_ENV_W64_2048: at the plain instances' 168 VGPRs the copy
// spills and costs more than the resident team).  The row pointer and the bin scale are extra
// arguments of those instances alone.
constexpr int kEnvBins = 128;   // MIMO_ENV_BINS
constexpr int kEnvFixed = 4;    // MIMO_ENV_FIXED

// Soft instances (MIMO_MODE_SOFT): the same trial, the same
// counts, and per trial a row of n_idx kSoftBins doubles (include/mimo_engine.h
// mimo_engine_soft_points): for every counter index the histogram of the 2 hb bit reliabilities of
// every valid slot, taken on the value that index slices -- the clean run's z_c, an iteration's
// z - dist -- by softbits.h soft_axis / soft_bin (max-log soft bit of each Gray bit of each axis,
// signed by the transmitted bit, 256 linear bins over +-rho_max).  Only where the index is recorded
// (a uniform branch): one ds_add_u32 per reliability into a per-team LDS histogram of kSoftBins
// uint32 (1 KiB), which the team stores as doubles to row[idx kSoftBins + ...] after `record` and
// zeroes again (plain stores, every cell written once, no global atomics).  All of it sits in the
// receiver phase, outside the antenna loop.  The row pointer and the bin scale 128 / rho_max are
// extra arguments of those instances alone.

// Coded instances (MIMO_MODE_CODED): the same trial, the same counts, and per trial and recorded
// counter index the quantised reliability c (softbits.h coded_value: an odd integer in [-63, 63],
// include/mimo_engine.h mimo_engine_coded_points) of every Gray bit of every valid slot, taken on the
// value that index slices, as one int8 at chan[(block n_idx + idx) S 2 hb + j S + k]: bit j of
// sub-carrier k, the I axis MSB first, then Q.  Plain byte stores from the receiver phase, every cell
// written once, no LDS and no barrier on top of the plain instance's.  The LDPC decoder (ldpc.hip)
// reads the buffer after the launch.  The buffer and the scale 32 / rho_max are extra arguments of
// those instances alone.

// Turbo instances (MIMO_MODE_TURBO): the same trial, the same counts, and per trial the AGC'd received
// vector z -- what CNC iteration 0 slices -- of every valid slot as one complex128 at
// zbuf[block S + k], sub-carrier order k.  Plain 16-byte stores from the receiver phase, where z is
// formed; every cell written once, no LDS and no barrier on top of the plain instance's.  The step
// kernel (turbo.hip; include/mimo_engine.h mimo_engine_turbo_points) reads the buffer after the
// launch.  The buffer is an extra argument of those instances alone.

constexpr int kMaxCsiAnt = 512;  // CSI-error runs: antennas (dynamic LDS per team, A doubles; engine.hip checks)
constexpr uint32_t kFixedCsiTrial = 0xFFFFFFFFu;  // CSI stream counter of fixed-channel runs (oracle/sim.py draws)
// The measured alternatives of the choices below (channel pipeline on / off per precision,
// register diet from F 8192, raw-word pipeline, alpha by library exp / erfc, shfl vs DPP
// sums) are in DESIGN.md §3 and profiles/r02/ab/; the losing variants were removed.

template <typename R>
struct TrialParams {
  using C = cx<R>;
  uint64_t seed;
  uint64_t first_trial;
  uint32_t* counts;              // [n_trials][n_idx]
  const C* tw;                   // team-FFT stage twiddles of (F, T) (team_fft.h fft_tw_off)
  const C* tw_wave;              // wave-split FFT twiddles of (F, T) (wave_fft.h), or null
  const R* ant_rel;              // [A]  d0 / d_a      (Rayleigh FSPL, relative)
  const R* f_rel;                // [S]  fc / f_k      (f_k float32-quantised as in the reference)
  const double* f_over_c;        // [S]  f_k / c       (LoS / two-path phases)
  const double* tx_pos;          // [A*3]
  const double2* lut;            // [kLut64] fp64 ln / sincos tables (real.h; fp64 instances only)
  const C* chan_tab;             // CH_TABLE: in-band channels [entries][A][S] (sub-carrier order k), see chan_period
  int n_ant, n_sc, qam_l, half_bits;
  uint32_t label_mask;
  int pa_kind, cnc_pa_kind;
  R sat_tx, sqrt_sat_tx, inv_sat_tx, rapp_p, toi_tx;
  R sat_cnc, sqrt_sat_cnc, inv_sat_cnc, toi_cnc, inv_alpha_cnc;
  R alpha_c;                     // 10^(IBO/10) S / A : gamma_a^2 = alpha_c / vk_pow[a]
  // alpha(gamma_a^2) as a degree-8 polynomial in x = vk_pow[a] A / S - 1 on |x| <= alpha_xlim
  // (host Chebyshev fit, ~1e-7 relative); the exact formula outside (engine.hip fit_alpha).
  // fp32 instances only: the fp64 instances always evaluate the exact formula.
  R apoly[9];
  R inv_vk0, alpha_xlim;
  R inv_vk0_f;                   // inv_vk0 F (the fp64 register-diet array pass sums vk / F)
  // fp64 instances: alpha(gamma_a^2) as a degree-18 polynomial in x on |x| <= alpha_xlim
  // (the host's Chebyshev interpolant at 64 nodes in long double, as monomials: Horner,
  // <= 1.6e-16 relative; the singularity of alpha(g0^2 / (1 + x)) at x = -1 is 4
  // half-widths away), the exact formula outside.
  double amono64[19];
  R es_over_snr;                 // Es / 10^(SNR/10)
  R csi_a, csi_b;                // sqrt(1 - eps^2), eps
  R inv_sqrt_f;
  int receiver;
  int max_iter;                  // largest iteration index to run (CNC / MCNC)
  uint32_t rec_mask;             // bit i: record iteration i
  int incl_clean, n_idx;
  double rx_x0, rx_z, rx_var, d0; // LoS / two-path geometry
  uint32_t ablate;               // diagnostic builds only (-DMIMO_ABLATION), see ABL_* below
  // Multi-point launches (mimo_engine_run_points): the kernel argument carries the table;
  // block b runs trial points[i].first_trial + b - point_start[i] of point i, where
  // point_start[i] <= b < point_start[i + 1].  The per-point parameters (PA, AGC, noise,
  // seed ...) are read from points[i] through the constant address space (scalar loads).
  const TrialParams* points;     // [n_points] (device)
  const uint32_t* point_start;   // [n_points + 1] block offsets (device)
  int n_points;
  uint32_t chan_period;          // 0, or the channel-replay period (mimo_config.chan_replay_period);
                                 // CH_TABLE: the entries of chan_tab (trial i reads entry i mod
                                 // chan_period), or 0: one entry per block of the launch
  // Last, so that the fields the antenna loop reloads keep their 16-byte alignment (the
  // scalar loads pair them as s_load_dwordx4; inserted after `seed` it cost the F 4096
  // instance 1 %, profiles/r04/misc/).
  uint64_t csi_seed;             // CH_TABLE + CSI: key of the one shared estimate (mimo_config.csi_seed)
};

// Ablation switches for cost breakdowns.  Compiled in only with -DMIMO_ABLATION
// (libmimo_engine_ablation.so); the production kernel has none of these branches.
enum : uint32_t { ABL_RNG = 1, ABL_FFT = 2, ABL_PASS1 = 4, ABL_PA = 8, ABL_XCHG = 16 };
#ifdef MIMO_ABLATION
#define MIMO_ABL(p, bit) (((p).ablate & (bit)) != 0)
#elif defined(MIMO_STATIC_ABLATE)  // ISA inspection only (tools/stage_hist.py): stages compiled out
#define MIMO_ABL(p, bit) ((MIMO_STATIC_ABLATE & (bit)) != 0)
#else
#define MIMO_ABL(p, bit) false
#endif

}  // namespace mimo
