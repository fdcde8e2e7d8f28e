/* mimo_engine.h -- C ABI of the MI355X Monte-Carlo BER engine (libmimo_engine.so).
 *
 * This is the drop-in boundary for the reference's hot path
 * (MarcinWachowiak/m-mimo-ofdm-with-nonlinear-pa-sim).  The reference is pure Python
 * with no FFI; the entry points below are what its object API binds to through ctypes
 * (see INTEGRATION.md), one group per reference seam:
 *
 *   coarse seam  mp_model.Link                    mp_model.py:32-329
 *     mimo_engine_create        <- Link.__init__                       mp_model.py:32-87
 *     mimo_engine_set_point     <- Link.update_distortion / set_snr    mp_model.py:230-251
 *     mimo_engine_run           <- Link.simulate (trial loop)          mp_model.py:89-228
 *     mimo_engine_measure_points   the same trials with signal / distortion power sums (SDR, EVM)
 *     mimo_engine_spectrum_points  the same trials with the array's radiated PSD per FFT bin
 *                                  (out-of-band emission, Bussgang gain, efficiency)
 *     mimo_engine_beam_points      the same trials with the signal, distortion and out-of-band power
 *                                  the array radiates towards a list of probe positions (beampattern)
 *     mimo_engine_envelope_points  the same trials with the distribution of the instantaneous power at
 *                                  every antenna's PA input and output (CCDF / PAPR, compression)
 *     mimo_engine_soft_points      the same trials with the histogram of the demapper's bit reliabilities
 *                                  per counter index (BICM GMI / achievable rate per CNC / MCNC iteration)
 *     mimo_engine_coded_points     the same trials with the bit and frame errors of an LDPC-coded link after
 *                                  a layered min-sum decoder, per counter index (coded BER / FER per iteration)
 *     mimo_engine_turbo_points     the same trials with the decoder in the CNC loop: the LDPC decoder's
 *                                  decisions, not hard slices, re-synthesise the distortion (errors per pass)
 *     mimo_engine_set_channel_bank  a table engine's bank of channel matrices, one per trial (snapshots)
 *     mimo_engine_set_tdl           the power-delay profile of a tapped-delay-line Rayleigh channel, drawn
 *                                   per trial on the device (frequency-selective fading)
 *     mimo_engine_set_rays          the same engine on a ray-cluster profile: every tap a sum of rays with
 *                                   caller-given steering vectors (spatially correlated taps, specular rays)
 *     mimo_engine_run_points    <- the drivers' grid loops over (IBO, Eb/N0), one launch
 *                                  for many points   main_mp_miso_cnc_constant_ber_req_ebn0_vs_ibo.py:100-215
 *   fine seams (float64 stage kernels, caller-owned host arrays)
 *     mimo_qam_map              <- modulation.modulate                 modulation.py:13-25
 *     mimo_qam_slice            <- demodulate / symbol_detection       modulation.py:63-88,138-146
 *     mimo_qam_llr              <- soft_decoding                       modulation.py:29-59
 *     mimo_qam_softbits            the soft mode's max-log soft bit lambda (no reference entry point)
 *     mimo_ldpc_decode             the coded mode's LDPC decoder on caller-given channel values
 *     mimo_engine_cnc_step         the turbo mode's step kernel on caller-given received vectors and decisions
 *     mimo_ofdm_tx / _rx        <- _tx_ofdm_symbol / _rx_ofdm_symbol   modulation.py:248-293
 *     mimo_fft                  <- utilities.to_freq/time_domain       utilities.py:311-339
 *     mimo_pa                   <- SoftLimiter/Rapp/ThirdOrderNonLin.process  distortion.py
 *     mimo_calc_alpha           <- Modem.calc_alpha                    modulation.py:178-189
 *     mimo_mrt_precode          <- AntennaArray.set_precoding_matrix   antenna_array.py:162-185
 *     mimo_combine              <- Miso*Fd.propagate                   channel.py:74-89,277-292
 *     mimo_awgn                 <- Awgn.process                        noise.py:45-83
 *     mimo_tdl_channels            the TDL engine's channel realisations (no reference entry point)
 *     mimo_rays_channels           ... and those of its ray-cluster profile
 *     mimo_count_bit_errors     <- utilities.count_mismatched_bits     utilities.py:94-104
 *     mimo_cnc_receive          <- CncReceiver.receive                 corrector.py:52-112
 *     mimo_cnc_receive_ex       <- CncReceiver.receive(return_bits=False) corrector.py:80-84
 *
 * Conventions: complex arrays are interleaved (re, im) doubles; sizes are element
 * counts; functions return 0 on success and a negative MIMO_E* code on error, with a
 * message from mimo_last_error() (thread-local).  No HIP call happens before the first
 * compute call, so a Python parent may create engines and fork workers (the
 * reference's drivers fork after building Link, main_mp_miso_cnc_ber_vs_ebn0.py:124-132).
 */
#ifndef MIMO_ENGINE_H
#define MIMO_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIMO_ABI_VERSION 8

enum { MIMO_OK = 0, MIMO_EINVAL = -1, MIMO_EHIP = -2, MIMO_ENOKERNEL = -3, MIMO_ENOMEM = -4 };
enum { MIMO_PA_NONE = 0, MIMO_PA_SOFTLIM = 1, MIMO_PA_RAPP = 2, MIMO_PA_TOI = 3 };
enum { MIMO_CH_RAYLEIGH = 1, MIMO_CH_LOS = 2, MIMO_CH_TWOPATH = 3, MIMO_CH_TABLE = 4, MIMO_CH_TDL = 5 };
enum { MIMO_RX_CNC = 1, MIMO_RX_MCNC = 2 };
enum { MIMO_PREC_F64 = 0, MIMO_PREC_F32 = 1 };

typedef struct mimo_engine mimo_engine;

/* System description: everything Link deep-copies at construction.  Arrays are copied.
 *
 * mimo_engine_create checks the description host-side, before any HIP call; one that breaks a
 * rule gives a null engine and MIMO_EINVAL with a message that names the field.  Next to the
 * ranges noted at the fields, the geometry:
 *   tx_pos            required; all 3 n_ant values finite
 *   rx_pos            finite
 *   rx_loc_var        finite and >= 0
 *   carrier_freqs     required; all n_fft values finite and > 0
 *   chan_table        MIMO_CH_TABLE: required; all 2 n_ant n_fft values finite
 * One rule is about what a run divides by, and is checked by mimo_engine_run and every *_points
 * call instead (MIMO_EINVAL, before any HIP call; an engine that is never run may hold it):
 *   tx_pos, rx_pos    every channel but MIMO_CH_TABLE (which reads no position): no antenna at
 *                     rx_pos -- the distance of the Rayleigh attenuation must be finite and > 0;
 *                     MIMO_CH_LOS and MIMO_CH_TWOPATH also: no antenna at (rx_pos[0], rx_pos[0],
 *                     rx_pos[2]), the centre the jitter is drawn around (both jittered coordinates
 *                     start from rx_pos[0], as mp_model.py:192-199 draws them) */
typedef struct mimo_config {
  int32_t n_ant;            /* antennas (AntennaArray.n_elements)                   */
  int32_t n_sub_carr;       /* data sub-carriers S (multiple of 4, S <= n_fft - 2)  */
  int32_t n_fft;            /* FFT size F: power of two, 128 ... 8192               */
  int32_t constel_size;     /* square QAM order M (4 ... 4096)                      */
  int32_t cp_len;           /* cyclic prefix (BER-neutral: memoryless PA, circular channel) */
  int32_t channel_kind;     /* MIMO_CH_* (TABLE: a fixed matrix, see chan_table, or a bank of them,
                               mimo_engine_set_channel_bank; TDL: a tapped-delay-line Rayleigh channel
                               per trial, mimo_engine_set_tdl -- reroll_chan must be 1 and chan_table
                               is not read)                                           */
  int32_t receiver_kind;    /* MIMO_RX_*                                            */
  int32_t device;           /* HIP device ordinal, -1 = current                      */
  double rx_pos[3];         /* nominal RX position [m]                               */
  double rx_loc_var;        /* LoS / two-path RX jitter span [m] (mp_model.py:192-199) */
  int32_t reroll_chan;      /* 1: per-trial channel reroll (Link.simulate reroll_chan) */
  int32_t precision;        /* MIMO_PREC_F64 (0, default: the reference's complex128 /
                               float64, modulation.py:270) or MIMO_PREC_F32 (fast variant) */
  const double* tx_pos;     /* [n_ant][3] antenna positions [m]                      */
  const double* carrier_freqs; /* [n_fft] carrier frequencies [Hz] in FFT-bin order  */
  const double* chan_table; /* MIMO_CH_TABLE only: [n_ant][n_fft] complex channel matrix
                               (Miso*Fd.channel_mat_fd), the same for every trial -- what
                               Link.simulate(reroll_chan=False) uses (mp_model.py:190-206) */
  int32_t chan_replay_period; /* 0 (default): an independent Rayleigh channel per trial.
                               > 0 (diagnostic, Rayleigh only): trial i draws the channel of
                               trial i mod period, emulating the reference's workers that all
                               replay one seeded channel sequence (channel.py:209-212);
                               bits and noise stay per trial.  Used to size the published
                               curves' channel variance (tests/test_gpu_link.py).  (ABI 5) */
  uint64_t csi_seed;        /* MIMO_CH_TABLE with CSI error: Philox key of the one erroneous
                               estimate every trial and every run shares -- Link.__init__ draws it
                               once from its noise generator, default_rng(0) (mp_model.py:74,87,272), so the
                               workers of a point see the same estimate whatever their seeds.
                               0: the run's seed (ABI 5 behaviour).  (ABI 6) */
} mimo_config;

/* Grid-point parameters: what Link keeps in its PA / receiver / noise objects.
 *
 * mimo_engine_set_point and every *_points call check each point host-side, before any HIP
 * call; a point that breaks a rule is MIMO_EINVAL with a message that names the field:
 *   ibo_db, snr_db    finite (snr_db = 1000 is a noiseless run); avg_symbol_power / 10^(snr_db / 10),
 *                     the noise power, must be finite too
 *   avg_symbol_power  finite and > 0
 *   pa_kind, cnc_pa_kind  MIMO_PA_NONE ... MIMO_PA_TOI, on every engine
 *   sat_pow           > 0 where pa_kind is softlim or rapp (+inf: a PA that never saturates);
 *                     not read otherwise (the TOI drivers send 0)
 *   toi_coeff         finite where pa_kind is toi; not read otherwise
 *   p_hardness        finite and > 0 where pa_kind, or under a CNC receiver cnc_pa_kind, is rapp:
 *                     the one hardness of both Rapp models
 *   cnc_sat_pow       > 0 where the engine's receiver is MIMO_RX_CNC and cnc_pa_kind is softlim or rapp
 *   cnc_toi_coeff     finite where the receiver is MIMO_RX_CNC and cnc_pa_kind is toi
 *   cnc_alpha         finite and non-zero
 *   csi_eps           a number < 1; NaN is refused, not read as perfect CSI
 *   array_alpha       finite and >= 0
 * The MCNC receiver re-transmits through the array's PA and reads none of cnc_pa_kind,
 * cnc_sat_pow, cnc_toi_coeff and cnc_alpha: any values that pass the rules above give the same counts. */
typedef struct mimo_point {
  double ibo_db;            /* IBO used by the per-antenna Bussgang AGC (mp_model.py:315-317) */
  double snr_db;            /* Link.set_snr value                                    */
  double avg_symbol_power;  /* Es = mean |C|^2 (modulation.py:218)                    */
  int32_t pa_kind;          /* array PA model                                        */
  int32_t cnc_pa_kind;      /* CNC receiver's PA copy                                */
  double sat_pow;           /* array PA saturation power (softlim / rapp)            */
  double p_hardness;        /* Rapp p                                                */
  double toi_coeff;         /* array PA cubic coefficient (toi)                      */
  double cnc_sat_pow;       /* CNC PA saturation power                                */
  double cnc_toi_coeff;     /* CNC PA cubic coefficient                               */
  double cnc_alpha;         /* CNC alpha (corrector.py:106-110)                      */
  double csi_eps;           /* CSI error epsilon; < 0 = perfect CSI.  With CSI error: n_ant <= 512,
                               and the run fails with MIMO_EINVAL (before any launch) if the
                               instance's static LDS plus the n_ant-real power table exceed the
                               CU's LDS (round 6)                                    */
  double array_alpha;       /* 0: each antenna's Bussgang gain from its precoding power
                               (Link, mp_model.py:315-317).  > 0: that gain for every antenna --
                               the TOI drivers' measured alpha_estimate
                               (main_miso_cnc_ber_vs_ebn0_toi.py:95-121,247-249).  Not with the
                               float32 F = 8192 instance (MIMO_EINVAL).  (ABI 8) */
} mimo_point;

int32_t mimo_abi_version(void);
const char* mimo_last_error(void);
int32_t mimo_device_count(void);

/* Coarse seam ------------------------------------------------------------------- */
mimo_engine* mimo_engine_create(const mimo_config* cfg);
int32_t mimo_engine_set_point(mimo_engine* e, const mimo_point* pt);
/* Runs trials [first_trial, first_trial + n_trials) of the point, keyed by `seed`.
 * iters: sorted, unique receiver iterations to record (0 = standard RX), each in [0, 31].
 * Counter layout (mp_model.py:127-131,217-222): [clean if incl_clean] + one per iter.
 * err_out / bits_out: n_idx totals (ADDED to, like the reference's shared counters).
 * per_trial: optional [n_trials][n_idx] bit-error counts, NULL to skip. */
int32_t mimo_engine_run(mimo_engine* e, uint64_t seed, uint64_t first_trial, uint64_t n_trials,
                        const int32_t* iters, int32_t n_iters, int32_t incl_clean,
                        uint64_t* err_out, uint64_t* bits_out, uint32_t* per_trial);
/* Many grid points of the same system in one go (BASELINE config 4 sweeps): point i runs
 * trials [first_trial[i], first_trial[i] + n_trials[i]) keyed by seeds[i] with the
 * parameters points[i].  Every point's trials are a contiguous block range of one kernel
 * launch (launches hold up to 2^20 trials), so a grid of small points fills the GPU.
 * All points share iters / incl_clean and must agree on CSI error on / off.
 * err_out / bits_out: [n_points][n_idx] totals (ADDED to).  per_trial: optional
 * [sum n_trials][n_idx] counts in point order, NULL to skip.  mimo_engine_run(...) is
 * this call with the engine's current point. */
int32_t mimo_engine_run_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                               const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                               int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                               uint32_t* per_trial);
/* Measure mode (float64 engines): the trials, arguments, launch splitting and point rules of
 * mimo_engine_run_points and the same counts, plus per point a row of
 * n_meas = MIMO_MEAS_FIXED + n_idx power sums over the S data sub-carriers k of every trial:
 *   [0] Es  = sum |s_k|^2               s: the transmitted constellation point
 *   [1] Ez0 = sum |z0_k|^2              z0 = r / g: the AGC'd received value without noise
 *   [2], [3] Re, Im of C = sum z0_k conj(s_k)
 *   [4] Ed0 = sum |z0_k - s_k|^2
 *   [5 + i] Ee_i = sum |v_{i,k} - s_k|^2   v_i: the slicer input of counter index i (counts
 *                                       layout: the clean run's z_c, an iteration's z - dist)
 * from which gain C / Es, SDR |C|^2 / (Es Ez0 - |C|^2), slicer SDR Es / Ed0 and per-iteration
 * SNDR Es / Ee_i follow.  meas_out: [n_points][n_meas] totals (ADDED to; summed in a fixed
 * order: equal calls return equal bits).  per_trial_meas: optional [sum n_trials][n_meas]
 * rows in point order, NULL to skip.  A float32 engine or a null meas_out is MIMO_EINVAL,
 * before any HIP call.  (Added within ABI 8: a library without it is reported by name.) */
enum { MIMO_MEAS_FIXED = 5 };
int32_t mimo_measure_width(int32_t n_iters, int32_t incl_clean); /* MIMO_MEAS_FIXED + n_idx; host only */
int32_t mimo_engine_measure_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                   const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                   int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                   uint32_t* per_trial, double* meas_out, double* per_trial_meas);
/* Spectrum mode (float64 engines): the trials, arguments and point rules of mimo_engine_run_points
 * and the same counts, plus per point a row of n_spec = n_fft + MIMO_SPEC_FIXED sums over what the
 * array radiates in the main transmission of every trial, with Y_a = FFT(PA(IFFT(X_a))) of antenna
 * a (ortho transform pair) and X_a = s conj(Hhat_a) / ||Hhat|| its precoded input (the estimate
 * under CSI error):
 *   [k], k < n_fft     psd[k] = sum_a |Y_a[k]|^2, FFT bin k in numpy.fft order (bin 0 = DC), so
 *                      sum_k psd[k] = sum_a sum_n |y_a[n]|^2, the radiated power
 *   [n_fft]            Ex = sum_a sum_{k in band} |X_a[k]|^2   (= sum_k |s_k|^2 under MRT)
 *   [n_fft + 1], [+ 2] Re, Im of C = sum_a sum_{k in band} Y_a[k] conj(X_a[k])
 * from which the out-of-band share, the array's Bussgang gain C / Ex and its efficiency
 * sum psd / Ex follow.  MCNC re-transmissions and the CNC receiver's chain do not contribute.
 * spec_out: [n_points][n_spec] totals (ADDED to; summed in a fixed order: equal calls return equal
 * bits).  per_trial_spec: optional [sum n_trials][n_spec] rows in point order, NULL to skip; they
 * do not depend on how the call is split into launches.  The per-trial rows of one launch live in
 * a device buffer of at most MIMO_SPEC_BUFFER_BYTES (256 MiB, a design figure), so a spectrum
 * launch holds floor(2^28 / (8 n_spec)) trials -- 4,094 at n_fft 8192, 129,553 at 256 -- or
 * fewer (MIMO_MAX_LAUNCH_TRIALS).  A float32 engine or a null spec_out is MIMO_EINVAL, before any
 * HIP call.  (Added within ABI 8: a library without it is reported by name.) */
enum { MIMO_SPEC_FIXED = 3 };
#define MIMO_SPEC_BUFFER_BYTES (256u << 20)
int32_t mimo_spectrum_width(int32_t n_fft); /* n_fft + MIMO_SPEC_FIXED; host only, EINVAL for a bad n_fft */
int32_t mimo_engine_spectrum_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                    const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                    int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                    uint32_t* per_trial, double* spec_out, double* per_trial_spec);
/* Beam mode (float64 engines): the trials, arguments and point rules of mimo_engine_run_points and
 * the same counts, plus per point and per probe position q (n_probes 3-D points [m], the same for
 * every point of the call) MIMO_BEAM_FIXED sums over what the array radiates towards q in the main
 * transmission of every trial.  With G_q[a,k] = exp(+j 2 pi d_qa f_k / c) c / (4 pi d_qa f_k) the
 * line-of-sight channel from antenna a to the probe at FFT bin k (d_qa their distance, f_k =
 * carrier_freqs[k], gain 0 dB), Y_a and X_a as in the spectrum mode, R_q[k] = sum_a G_q[a,k] Y_a[k]
 * the field at the probe and U_q[k] = sum_a G_q[a,k] X_a[k] its linear part's source:
 *   [0] Py_in  = sum_{k in band} |R_q[k]|^2
 *   [1] Py_oob = sum_{k not in band} |R_q[k]|^2      (DC and Nyquist included)
 *   [2] Px     = sum_{k in band} |U_q[k]|^2
 *   [3], [4] Re, Im of C = sum_{k in band} R_q[k] conj(U_q[k])
 * from which the Bussgang gain C / Px towards q, the signal |C|^2 / Px, the uncorrelated in-band
 * distortion Py_in - |C|^2 / Px and the out-of-band pattern follow.  MCNC re-transmissions and the
 * CNC receiver's chain do not contribute.  beam_out: [n_points][n_probes][MIMO_BEAM_FIXED] totals
 * (ADDED to; summed in a fixed order: equal calls return equal bits).  per_trial_beam: optional
 * [sum n_trials][n_probes][MIMO_BEAM_FIXED] rows in point order, NULL to skip; they do not depend
 * on how the call is split into launches.  The chains of one launch live in a device buffer of
 * 32 n_ant n_fft bytes per trial and at most MIMO_BEAM_BUFFER_BYTES (1 GiB, a design figure) in
 * all, so a beam launch holds floor(2^30 / (32 n_ant n_fft)) trials -- 256 at n_ant 64, n_fft
 * 2048 -- or fewer: the per-trial rows of a launch (40 n_probes bytes per trial) fill at most
 * MIMO_BEAM_ROWS_BYTES (256 MiB; 1,638 trials at 4,096 probes), and MIMO_MAX_LAUNCH_TRIALS lowers
 * the count further.  MIMO_EINVAL, before any HIP call: a float32 engine,
 * null probes or beam_out, n_probes outside [1, MIMO_BEAM_MAX_PROBES], a probe coordinate that is
 * not finite, a probe at an antenna's position, a system of which one trial does not fit the
 * buffer.  (Added within ABI 8: a library without it is reported by name.) */
enum { MIMO_BEAM_FIXED = 5, MIMO_BEAM_MAX_PROBES = 4096 };
#define MIMO_BEAM_BUFFER_BYTES (1ull << 30)
#define MIMO_BEAM_ROWS_BYTES (256u << 20)
int32_t mimo_beam_width(int32_t n_probes); /* n_probes MIMO_BEAM_FIXED; host only, EINVAL for a bad n_probes */
int32_t mimo_engine_beam_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                uint32_t* per_trial, const double* probes, int32_t n_probes, double* beam_out,
                                double* per_trial_beam);
/* Envelope mode (float64 engines): the trials, arguments, launch splitting and point rules of
 * mimo_engine_run_points and the same counts, plus per point a row of
 * n_env = 2 MIMO_ENV_BINS + MIMO_ENV_FIXED = 260 sums over the main transmission of every trial, over
 * all antennas a and all n_fft time samples n, with x_a[n] the PA input -- the ortho IFFT of the
 * precoded input X_a, as the spectrum mode defines X_a -- and y_a[n] = PA(x_a[n]):
 *   [b], b < 128       hist_in[b]: the number of samples whose |x_a[n]|^2 falls in bin b
 *   [128 + b]          hist_out[b]: the same for |y_a[n]|^2
 *   [256]              Pin = sum |x|^2
 *   [257]              Pout = sum |y|^2
 *   [258], [259]       Re, Im of C = sum y conj(x)
 * (by Parseval the three fixed sums equal the spectrum mode's Ex, sum_k psd[k] and C), from which
 * the CCDF of the instantaneous power before and after the PA, the PAPR at a probability, the
 * efficiency Pout / Pin and the Bussgang gain C / Pin follow.  The bins are floating-point bins,
 * defined on the bits of a double so that the device and any reference compute them with the same
 * integer operation: with scale = 1.0625 / ref_pow formed once on the host in double and
 * v = pw scale, pw = re re + im im of the sample,
 *   bin = clamp((bits(v) >> 49) - 8088, 0, 127),   8088 = (1023 - 12) << 3
 * -- 8 linear sub-bins per octave over 16 octaves; bin 0 also takes everything below (0 included),
 * bin 127 everything above (+inf included).  The lower edge of bin b >= 1 in units of
 * u = |.|^2 / ref_pow is 2^(-12 + b/8) (1 + (b%8)/8) 16/17 (integer division): about -36.4 dB to
 * +11.5 dB in steps of 0.28 to 0.51 dB.  The factor 17/16 keeps round figures off the edges: a soft
 * limiter puts every clipped sample at exactly sat_pow, which with ref_pow the mean power is
 * u = 10^(IBO/10), and u = 10^(i/10) for every integer i in [-3, 9] dB lies at least 0.8 % inside a
 * bin (IBO 0 dB would sit on the edge u = 1 without it).  MCNC re-transmissions and the CNC
 * receiver's chain do not contribute.  env_out: [n_points][n_env] totals (ADDED to; the histogram
 * cells are integers held exactly in doubles -- a trial has at most 2^25 samples -- so they are
 * bit-identical whatever the order or split; the fixed sums are summed in a fixed order: equal calls
 * return equal bits).  per_trial_env: optional [sum n_trials][n_env] rows in point order, NULL to
 * skip; they do not depend on how the call is split into launches.  The per-trial rows of one launch
 * live in a device buffer of at most MIMO_ENV_BUFFER_BYTES (256 MiB, a design figure), so an
 * envelope launch holds floor(2^28 / (8 n_env)) = 129,055 trials, or fewer
 * (MIMO_MAX_LAUNCH_TRIALS).  MIMO_EINVAL, before any HIP call: a float32 engine, a null env_out,
 * a ref_pow that is not finite or not > 0, or whose 1.0625 / ref_pow is not finite or not > 0.
 * (Added within ABI 8: a library without it is reported by name.) */
enum { MIMO_ENV_BINS = 128, MIMO_ENV_FIXED = 4 };
#define MIMO_ENV_BUFFER_BYTES (256u << 20)
int32_t mimo_envelope_width(void);              /* 2 MIMO_ENV_BINS + MIMO_ENV_FIXED = 260; host only */
int32_t mimo_envelope_edges(double* edges_out); /* MIMO_ENV_BINS - 1 lower edges of bins 1..127, as u; host only */
int32_t mimo_engine_envelope_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                    const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                    int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                    uint32_t* per_trial, double ref_pow, double* env_out, double* per_trial_env);
/* Soft mode (float64 engines): the trials, arguments, launch splitting and point rules of
 * mimo_engine_run_points and the same counts, plus per point and per counter index the histogram of
 * the demapper's bit reliabilities, from which the bit-wise mutual information of a coded link (the
 * BICM generalised mutual information, GMI) follows after every recorded CNC / MCNC iteration.
 *  Lattice and labels: the constellation in its own units (mimo_qam_map): levels are the odd integers
 *   -(L - 1) ... L - 1, L = sqrt(constel_size), hb = log2 L; a label is (gray(i_I) << hb) | gray(i_Q).
 *  Max-log soft bit: for a real coordinate x and Gray bit j of its axis, d0 = min |x - a| over the
 *   levels a whose Gray bit j is 0, d1 the same over those whose bit is 1, and
 *     lambda_j(x) = (d0 - d1) * (d0 + d1) * 0.25,
 *   each one IEEE double operation, no fused multiply-add anywhere.  Ties between levels do not
 *   change d0 or d1, so any method that finds the nearest level of each kind gives the same bits.
 *   lambda > 0 favours bit 1 (the sign of mimo_qam_llr); 4 lambda / noise_var is that seam's max-log
 *   approximation.
 *  Reliability and bin: for transmitted bit b, rho = lambda if b = 1, else -lambda; rho < 0 is a
 *   hard-decision error.  With scale = 128.0 / rho_max formed once on the host in double,
 *     bin = clamp(floor(rho * scale), -128, 127) + 128,
 *   the clamp in double before the integer conversion: 256 linear bins of width rho_max / 128, bin
 *   128 opens at exactly 0, bins 0 and 255 take everything beyond the range.
 *  Row of a trial: n_idx * MIMO_SOFT_BINS doubles, n_idx as in the counts layout ([clean if
 *   incl_clean] + one entry per recorded iteration).  Cell [i][b] is the number of the
 *   n_sub_carr log2(constel_size) bit reliabilities of counter index i that fall in bin b: both axes
 *   and every Gray bit of every data sub-carrier, pooled, taken on the value that index slices (the
 *   clean run's z_c, or an iteration's z - dist).  Only recorded iterations are binned; off-band
 *   slots contribute nothing.
 * soft_out: [n_points][n_idx * 256] totals (ADDED to; the cells are integers held exactly in doubles,
 * so totals are bit-identical whatever the order or split).  per_trial_soft: optional
 * [sum n_trials][n_idx * 256] rows in point order, NULL to skip.  The per-trial rows of one launch
 * live in a device buffer of at most MIMO_SOFT_BUFFER_BYTES (256 MiB, a design figure), so a soft
 * launch holds floor(2^28 / (8 * 256 * n_idx)) trials, or fewer (MIMO_MAX_LAUNCH_TRIALS).
 * MIMO_EINVAL, before any HIP call: a float32 engine, a null soft_out, a rho_max that is not finite
 * and > 0, or whose 128 / rho_max is not finite and > 0.  (Added within ABI 8: a library without it
 * is reported by name.) */
enum { MIMO_SOFT_BINS = 256 };
#define MIMO_SOFT_BUFFER_BYTES (256u << 20)
int32_t mimo_soft_width(int32_t n_iters, int32_t incl_clean); /* MIMO_SOFT_BINS * n_idx; host only */
int32_t mimo_engine_soft_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                uint32_t* per_trial, double rho_max, double* soft_out, double* per_trial_soft);
/* Coded mode (float64 engines): the trials, arguments, launch splitting and point rules of
 * mimo_engine_run_points and the same counts, plus per point and per counter index the bit and frame
 * errors of an LDPC-coded link after a real iterative decoder of finite length with fixed-point
 * messages, fed by the demapper's reliabilities after every recorded CNC / MCNC iteration.  There is
 * no encoder: the labels are i.i.d. uniform draws, that is a codeword of any linear code XORed with
 * a uniform scrambler known to the receiver, and a min-sum decoder is symmetric under the sign flips
 * of a codeword, so decoding the reliabilities rho (> 0: the transmitted bit is favoured) against
 * the all-zero codeword has exactly the error events of that scrambled coded link.  Everything is
 * integer after one floor, so any implementation of this text gives the same numbers.
 *  Code: a QC-LDPC code given by its base matrix (mimo_ldpc_code below; no table ships here).  z in
 *   [1, 512], n_rows in [1, 64], n_cols in [2, 128], N = n_cols z code bits; shifts[r][c] is -1 for a
 *   zero block, else s in [0, z): check i of base row r touches bit c z + (i + s) mod z of base
 *   column c.  Every base row has weight 2 ... 32, every base column weight >= 1.  n_dec_iters in
 *   [1, 64] decoder iterations, always run in full (no early stop).
 *  Channel value: with scale = 32.0 / rho_max formed once on the host in double and rho exactly the
 *   soft mode's reliability (mimo_engine_soft_points; no fused multiply-add),
 *     c = 2 * clamp(floor(rho * scale), -32, 31) + 1,
 *   the clamp in double before the integer conversion: an odd integer in [-63, 63], never 0; c < 0 is
 *   an uncoded bit error.  The 64 bins' edges are soft-mode edges at the same rho_max.
 *  Bit stream of one trial and counter index: Gray bit j of data sub-carrier k at p = j S + k, j in
 *   mimo_qam_llr's layout (the I axis MSB first, then the Q axis), k in the order of the labels,
 *   S = n_sub_carr.  n_cw = floor(S log2 M / N) codewords, >= 1; bit n of codeword w is stream
 *   position n n_cw + w (interleaved: every codeword sees every bit level); positions from n_cw N
 *   upwards are not decoded.
 *  Decoder: layered normalised min-sum, factor 3/4.  L[n] = c[n] (int16), one message R per edge,
 *   starting at 0.  n_dec_iters times, the base rows r in ascending order, and for every check i of
 *   row r (independent within a layer) and each of its edges e:  T_e = L[n_e] - R_e;  m_e = the
 *   smallest |T| over the other edges of the check;  sg_e = -1 if an odd number of the other edges
 *   have T < 0 (a T of 0 counts as non-negative), else +1;  R_e = sg_e min(127, (3 m_e) >> 2);
 *   L[n_e] = T_e + R_e.  No other clamp: L = c + the bit's current R's, |L| <= 63 + 127 n_rows <= 8191.
 *   Ties in the minimum change no value.  Hard decision: bit = 1 iff L < 0.
 *  Row of a trial: n_idx * MIMO_CODED_FIXED doubles, all integers; per counter index, over the trial's
 *   n_cw codewords: [0] the number of c < 0 among the n_cw N decoded positions, [1] the number of
 *   L < 0 after decoding, [2] codewords with any L < 0, [3] codewords whose hard decision has a
 *   non-zero syndrome.  (A flagged frame is no codeword, so it is wrong: [2] - [3] counts the frames
 *   that are wrong and pass every check, the undetected errors.)  Only recorded iterations leave cells.
 * coded_out: [n_points][n_idx * 4] totals (ADDED to; integers held exactly in doubles, so totals are
 * bit-identical whatever the order or split).  per_trial_coded: optional [sum n_trials][n_idx * 4]
 * rows in point order, NULL to skip.  per_trial_chan: optional [sum n_trials][n_idx][S log2 M] int8,
 * the c values of every stream position (the undecoded tail included), NULL to skip: any decoder of
 * the caller's can run on them.  The channel values of one launch live in a device buffer of at most
 * MIMO_CODED_BUFFER_BYTES (256 MiB, a design figure), so a coded launch holds
 * floor(2^28 / (n_idx S log2 M)) trials, or fewer (MIMO_MAX_LAUNCH_TRIALS).  The decoder keeps its
 * state in the LDS of one workgroup: 2 B per code bit (rounded up to 8) + 8 B per check + 96 B.
 * MIMO_EINVAL, before any HIP call, with a message naming the field: a float32 engine; a null code,
 * code->shifts or coded_out; a range above broken; N > S log2 M; a rho_max that is not finite and
 * > 0, or whose 32 / rho_max is not finite and > 0; a decoder state above 163,840 B (the message
 * names the figure).  (Added within ABI 8: a library without it is reported by name.) */
typedef struct mimo_ldpc_code {
  int32_t z;             /* lifting size, 1 ... 512 */
  int32_t n_rows;        /* base rows, 1 ... 64 */
  int32_t n_cols;        /* base columns, 2 ... 128; N = n_cols z code bits */
  const int16_t* shifts; /* [n_rows][n_cols]: -1 = zero block, else s in [0, z): check i of base
                            row r touches bit c z + (i + s) mod z of base column c */
  int32_t n_dec_iters;   /* 1 ... 64, always run in full: no early stop */
} mimo_ldpc_code;
enum { MIMO_CODED_FIXED = 4 };
#define MIMO_CODED_BUFFER_BYTES (256u << 20)
int32_t mimo_coded_width(int32_t n_iters, int32_t incl_clean); /* MIMO_CODED_FIXED * n_idx; host only */
/* n_cw = floor(n_sub_carr log2(constel_size) / N) >= 1, or MIMO_EINVAL (the code's rules, the
 * constellation, N > n_sub_carr log2 constel_size); host only */
int32_t mimo_coded_codewords(int32_t n_sub_carr, int32_t constel_size, const mimo_ldpc_code* code);
int32_t mimo_engine_coded_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                 const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                 int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                 uint32_t* per_trial, const mimo_ldpc_code* code, double rho_max, double* coded_out,
                                 double* per_trial_coded, int8_t* per_trial_chan);
/* Turbo mode (float64 engines with MIMO_RX_CNC; any channel kind, CSI error or PA at the transmitter):
 * the same trials, the same counts in the same order as mimo_engine_run_points, and per trial the
 * errors of the coded mode's LDPC-coded link in n_passes passes of a CNC receiver whose distortion
 * estimate is re-synthesised from the decoder's decisions instead of hard slices (decoder-in-the-loop
 * CNC).  The receiver's PA model is the point's cnc_pa_kind and its parameters, exactly as the fused
 * CNC loop uses them.  Everything is integer after the coded mode's one floor.  The code, rho_max, the
 * channel-value rule c = 2 clamp(floor(rho scale), -32, 31) + 1, the bit stream p = j S + k, the
 * codeword interleaving (bit n of codeword w at n n_cw + w), the decoder and the four cells are
 * those of mimo_engine_coded_points, unchanged.  n_passes in [1, 16].
 *  v_0 = z, the value CNC iteration 0 slices: r + sigma n scaled by 1 / g, in-band, in label order k.
 *  For pass q = 0 ... n_passes - 1:
 *   1. c_q is the stream of channel values of v_q, rho signed by the transmitted bits.
 *   2. The n_cw codewords are decoded to L_q; cells [q][0..3] are the coded mode's four cells on c_q, L_q.
 *   3. If q is the last pass, stop.  Else the decided bit of stream position p is b_tx XOR [L_q < 0] for
 *      p < n_cw N (the decoder's decision; L = 0 counts as non-negative) and b_tx XOR [c_q < 0] on the
 *      undecoded tail (the demapper's decision).  The decided label l_hat[k] has bit j of the stream
 *      as bit j of the label, MSB first: the I axis, then the Q axis.  s_hat = const[l_hat].
 *   4. dist = FFT(PA_cnc(IFFT(up(s_hat)))) / alpha_cnc - s_hat, both transforms ortho, up placing the
 *      symbols in the in-band bins: the CNC step of corrector.py:84-110 with s_hat in place of the slice.
 *   5. v_{q+1} = z - dist.
 *  Row of a trial: n_passes * MIMO_CODED_FIXED doubles, all integers.  Pass 0's cells are the coded
 *  mode's cells at CNC iteration 0, exactly.  If pass q decodes every frame correctly and the stream
 *  has no tail, the decisions are the transmitted labels and the rows of passes q + 1 and q + 2 are equal.
 * iters / incl_clean select the counts alone, as in every mode.
 * turbo_out: [n_points][n_passes * 4] totals (ADDED to; integers held exactly in doubles).
 * per_trial_turbo: optional [sum n_trials][n_passes * 4].  per_trial_chan: optional
 * [sum n_trials][n_passes][S log2 M] int8, c_q of every stream position.  per_trial_z: optional
 * [sum n_trials][S] complex128 (re, im), z.  The buffers of one launch count against one budget,
 * MIMO_TURBO_BUFFER_BYTES: per trial 16 S bytes of z, S log2 M bytes of channel values (times
 * n_passes only when per_trial_chan is asked for) and S log2 M bytes of decisions, so a turbo
 * launch holds floor(2^28 / (16 S + (1 or n_passes) S log2 M + S log2 M)) trials, or fewer
 * (MIMO_MAX_LAUNCH_TRIALS); per-trial results do not depend on the split.
 * mimo_engine_last_decode_ms covers the whole pass loop (step kernels and decoders).
 * MIMO_EINVAL, before any HIP call, with a message naming the field: every rule of the coded call;
 * a float32 engine; an engine whose receiver is not MIMO_RX_CNC; n_passes outside [1, 16]; a null
 * turbo_out.  (Added within ABI 8: a library without it is reported by name.) */
#define MIMO_TURBO_MAX_PASSES 16
#define MIMO_TURBO_BUFFER_BYTES (256u << 20)
int32_t mimo_turbo_width(int32_t n_passes); /* MIMO_CODED_FIXED * n_passes; host only */
int32_t mimo_engine_turbo_points(mimo_engine* e, int32_t n_points, const mimo_point* points, const uint64_t* seeds,
                                 const uint64_t* first_trial, const uint64_t* n_trials, const int32_t* iters,
                                 int32_t n_iters, int32_t incl_clean, uint64_t* err_out, uint64_t* bits_out,
                                 uint32_t* per_trial, const mimo_ldpc_code* code, double rho_max, int32_t n_passes,
                                 double* turbo_out, double* per_trial_turbo, int8_t* per_trial_chan,
                                 double* per_trial_z);
/* The seam of the turbo mode: steps 4 and 5 above by the production step kernel, with the engine's
 * tables and the point's derived parameters, on n caller-given vectors z_iq [n][S] complex128 (re, im)
 * and decided labels [n][S] in [0, M); v_out [n][S] complex128 = z - dist.  n in [0, 1048576] (2^20, one
 * launch; n = 0 touches nothing).  Float64 engines with MIMO_RX_CNC.  MIMO_EINVAL before any HIP call: a
 * float32 or MCNC engine, a null or invalid point, n outside that range, a null array, a label
 * outside [0, M).  (Added within ABI 8.) */
int32_t mimo_engine_cnc_step(mimo_engine* e, const mimo_point* point, const double* z_iq, const int32_t* labels,
                             int64_t n, double* v_out);
/* Channel bank (MIMO_CH_TABLE engines): many channel matrices on the device, one per trial.
 * tables is [n_bank][n_ant][n_fft] complex, each entry in chan_table's layout.  From then on trial i
 * (the absolute index, first_trial + offset) of mimo_engine_run and of every *_points call uses
 * table i mod n_bank.  n_bank = 0: back to the create-time table.  The tables are copied, their
 * in-band columns only (as mimo_engine_create keeps chan_table's), and uploaded at the next run: no
 * HIP call happens here.  A float32 engine stores float2, rounded to nearest.  The bank lives in a
 * device buffer of at most MIMO_BANK_BUFFER_BYTES (a design figure), so it holds
 * mimo_bank_capacity entries: 1,024 at n_ant 64, n_sub_carr 1024 in float64.  MIMO_EINVAL, with a
 * message naming the field: an engine that is not MIMO_CH_TABLE; null tables with n_bank > 0; a value
 * that is not finite (the message names the entry and the antenna); n_bank < 0 or above
 * mimo_bank_capacity.  One shared estimate per table is the table engine's CSI-error rule, and
 * per-entry estimates are not built: any run on an engine with n_bank > 1 whose points have
 * csi_eps >= 0 is MIMO_EINVAL, before any HIP call.  (Added within ABI 8: a library without it is
 * reported by name.) */
#define MIMO_BANK_BUFFER_BYTES (1ull << 30)
/* entries that fit: floor(MIMO_BANK_BUFFER_BYTES / (n_ant n_sub_carr (16 | 8 bytes))); host only,
 * MIMO_EINVAL for n_ant < 1, n_sub_carr < 1 or an unknown precision */
int64_t mimo_bank_capacity(int32_t n_ant, int32_t n_sub_carr, int32_t precision);
int32_t mimo_engine_set_channel_bank(mimo_engine* e, int32_t n_bank, const double* tables);
/* Tapped-delay-line (TDL) Rayleigh channel (MIMO_CH_TDL engines): a frequency-selective channel
 * drawn per trial and antenna from a caller-given power-delay profile.
 *  Taps: tap l < L of antenna a in trial i under the key seed:
 *   (w0, w1, ., .) = Philox4x32-10 of counter (l, i mod 2^32, 7, a) (stream 7; stream 6 is mimo_awgn's),
 *   u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32,
 *   g[a][l] = ant_amp[a] sqrt(powers[l]) sqrt(-ln u1) exp(j 2 pi u2)         (mimo_awgn's formula)
 *   -- a CN(0, ant_amp[a]^2 powers[l]) draw; the powers are used as given, not normalised.
 *  Frequency response at FFT bin n (numpy.fft order, bin 0 = the centre frequency):
 *   H[a][n] = sum_l g[a][l] W[(n delays[l]) mod n_fft],  summed in ascending l from 0,
 *   W[m] = exp(-j 2 pi m / n_fft) from a table the host builds once in double, W[0] = (1, -0.0 or
 *   0.0) exactly: a single tap at delay 0 gives H[a][n] = g[a][0] bit for bit.
 *  Engine: it selects the table instances of the trial kernel and needs a profile before its first
 *   run (MIMO_EINVAL without one); reroll_chan = 0 is refused by mimo_engine_create (a fixed channel
 *   is a table).  Before every trial-kernel launch of every call a generator kernel fills bank entry
 *   b with the realisation of the (point seed, trial) of the launch's block b, in-band columns only,
 *   in device memory; a float32 engine stores the values rounded to nearest.  A launch therefore
 *   holds at most mimo_bank_capacity trials and longer calls split; per-trial rows and counts do not
 *   depend on where.  Points with csi_eps >= 0 are MIMO_EINVAL, before any HIP call.
 *  mimo_engine_set_tdl copies the profile (no HIP call).  MIMO_EINVAL, with a message naming the
 *   field: an engine that is not MIMO_CH_TDL, a null profile, delays or powers, n_taps outside
 *   [1, 64], delays that are not strictly ascending in [0, n_fft), a power or an amplitude that is
 *   not finite and > 0.
 *  mimo_tdl_channels is the fine seam: the same realisations, by the same device function, on host
 *   arrays.  h_out is [n][n_ant][n_fft] complex, trial first_trial + j at h_out[j]; taps_out, optional,
 *   [n][n_ant][L] complex.  n_fft a power of two in [2, 8192], n_ant >= 1, n >= 0 (n = 0: MIMO_OK,
 *   nothing written); a null h_out is MIMO_EINVAL.
 * (Added within ABI 8: a library without them is reported by name.) */
typedef struct mimo_tdl {
  int32_t n_taps;          /* L, 1 ... 64 */
  const int32_t* delays;   /* [L] whole samples, strictly ascending, 0 <= d < n_fft */
  const double* powers;    /* [L] linear, finite and > 0 (used as given, not normalised) */
  const double* ant_amp;   /* [n_ant] amplitude per antenna, finite and > 0; NULL = 1 */
} mimo_tdl;
enum { MIMO_TDL_MAX_TAPS = 64 };
int32_t mimo_engine_set_tdl(mimo_engine* e, const mimo_tdl* prof);
int32_t mimo_tdl_channels(const mimo_tdl* prof, int32_t n_ant, int32_t n_fft, uint64_t seed, uint64_t first_trial,
                          int64_t n, double* h_out, double* taps_out);
/* Ray-cluster channel (MIMO_CH_TDL engines): the TDL channel with every tap a sum of rays, so that
 * the taps are correlated over the array.  Ray r has a caller-given steering vector steer[.][r]
 * over the antennas, belongs to tap ray_tap[r], and carries one complex gain per trial that all
 * antennas share: complex normal (diffuse) or of unit modulus (specular).  Tap l has the transmit
 * correlation R_l = S_l diag(ray_amp^2) S_l^H over its diffuse rays; one specular ray next to
 * diffuse ones makes it Rician; a single specular ray is a plane or spherical wave at a delay.
 *  Gains: ray r < R in trial i under the key seed:
 *   (w0, w1, ., .) = Philox4x32-10 of counter (r, i mod 2^32, 8, 0)  (stream 8; 7 is the TDL taps'),
 *   u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32,
 *   diffuse:   c_r = ray_amp[r] sqrt(-ln u1) exp(j 2 pi u2)     (the TDL tap's formula)
 *   specular:  c_r = ray_amp[r] exp(j 2 pi u2);
 *   the gain does not depend on the antenna.
 *  Taps: g[a][l] = sum over the rays r of tap l of c_r steer[a][r], each complex product four fused
 *   multiply-adds onto an accumulator that starts at 0, and the products added in the fixed order
 *   csrc/tdl.h documents (16 interleaved partial sums in ascending r, then a fixed binary tree); a
 *   tap of one ray with steer = 1 + 0j is the gain bit for bit.
 *  Response: H[a][n] = sum_l g[a][l] W[(n delays[l]) mod n_fft], exactly as for mimo_tdl.
 *  Engine: mimo_engine_set_rays is valid on a MIMO_CH_TDL engine only, copies the profile and makes
 *   no HIP call (the next run uploads the tables); whichever of mimo_engine_set_tdl and
 *   mimo_engine_set_rays was called last is the engine's profile.  Everything else about a TDL
 *   engine holds: the table instances, block b reads entry b, the mimo_bank_capacity split,
 *   csi_eps >= 0 refused, mimo_engine_last_chan_ms; a float32 engine stores the float64 response
 *   rounded to nearest.
 *  MIMO_EINVAL before any HIP call, with a message naming the field: an engine that is not
 *   MIMO_CH_TDL; a null profile, delays, ray_tap, ray_amp or steer; n_taps outside [1, 64] or n_rays
 *   outside [n_taps, 1024]; delays that break mimo_tdl's rule; a ray_tap that is not non-decreasing
 *   from 0 to n_taps - 1 in steps of 0 or 1; a ray_amp that is not finite and > 0; a ray_kind other
 *   than 0 or 1; a steer value that is not finite (the message names the antenna and the ray).
 *  mimo_rays_channels is the fine seam, by the engine's own kernel: h_out, taps_out, n_fft, n_ant and
 *   n as for mimo_tdl_channels; gains_out, optional, is [n][n_rays] complex.
 * (Added within ABI 8: a library without them is reported by name.) */
typedef struct mimo_rays {
  int32_t n_taps;            /* L, 1 ... 64 */
  const int32_t* delays;     /* [L] as in mimo_tdl */
  int32_t n_rays;            /* R, L ... 1024 (MIMO_RAYS_MAX) */
  const int32_t* ray_tap;    /* [R] tap of ray r: non-decreasing, ray_tap[0] = 0, steps of 0 or 1,
                                ray_tap[R-1] = L-1 (every tap has a ray, a tap's rays are contiguous) */
  const double* ray_amp;     /* [R] finite and > 0 */
  const uint8_t* ray_kind;   /* [R] 0 diffuse, 1 specular; NULL = all diffuse */
  const double* steer;       /* [n_ant][R] complex (re, im), all finite */
} mimo_rays;
enum { MIMO_RAYS_MAX = 1024 };
int32_t mimo_engine_set_rays(mimo_engine* e, const mimo_rays* prof);
int32_t mimo_rays_channels(const mimo_rays* prof, int32_t n_ant, int32_t n_fft, uint64_t seed, uint64_t first_trial,
                           int64_t n, double* h_out, double* taps_out, double* gains_out);
/* Device time of the trial kernels of the last run, in ms (HIP events on the engine stream). */
double mimo_engine_last_kernel_ms(const mimo_engine* e);
/* ... and of the beamforming kernels of the last beam call (0 after any other call). */
double mimo_engine_last_beam_ms(const mimo_engine* e);
/* ... and of the decoder kernels of the last coded call, or of the pass loop (step kernels and
 * decoders) of the last turbo call (0 after any other call). */
double mimo_engine_last_decode_ms(const mimo_engine* e);
/* ... and of the TDL generator kernels of the last call on a MIMO_CH_TDL engine (0 on any other);
 * an event pair of its own: mimo_engine_last_kernel_ms does not include it. */
double mimo_engine_last_chan_ms(const mimo_engine* e);
/* Which kernel instance the current config selects: "F=2048 T=128 slots=8 aligned ..." */
const char* mimo_engine_describe(const mimo_engine* e);
void mimo_engine_destroy(mimo_engine* e);

/* Fine seams (float64) ------------------------------------------------------------
 * Caller-owned host arrays; complex data as (re, im) pairs.  Every seam checks its sizes
 * host-side, before any allocation or HIP call: a value outside the ranges below is
 * MIMO_EINVAL with a message in mimo_last_error(), and a size of 0 (n, batch, n_cols) is
 * MIMO_OK with nothing read or written (mimo_count_bit_errors stores 0).
 *   constel_size  a square power of two in [4, 4096]: 4, 16, 64, 256, 1024, 4096
 *   n, batch      >= 0
 *   n_fft         a power of two in [2, 8192]
 *   n_sub_carr    even, in [2, n_fft - 2]
 *   cp_len        in [0, n_fft]
 *   n_ant         >= 1;  n_cols, n >= 0 (mimo_mrt_precode, mimo_combine: [n_ant][n] row-major)
 *   kind, pa_kind MIMO_PA_NONE ... MIMO_PA_TOI
 *   alpha         finite and non-zero (mimo_cnc_receive, mimo_cnc_receive_ex)
 *   iters         n_iters >= 1 values, ascending, unique, >= 0
 * mimo_qam_map: labels in [0, constel_size).  mimo_qam_llr: noise_var holds n values; out is
 * [n][log2 constel_size], MSB first, +inf where the zero-bit sum underflows to 0.
 * mimo_qam_softbits: out is [n][log2 constel_size] values of the soft mode's lambda (see
 * mimo_engine_soft_points), the I-axis bits MSB first and then the Q-axis bits: mimo_qam_llr's layout.
 * mimo_ofdm_tx: sym_iq [batch][n_sub_carr] -> td_iq [batch][n_fft + cp_len]; mimo_ofdm_rx the
 * reverse.  mimo_awgn: out = in + sqrt(-ln u1) exp(j 2 pi u2) noise_std / sqrt(2) with
 * (w0, w1, ., .) = Philox4x32-10 of counter (i_lo, counter_lo, 6, counter_hi ^ i_hi) under the
 * key seed for element i, u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32. */
int32_t mimo_qam_map(int32_t constel_size, const int32_t* labels, int64_t n, double* out_iq);
int32_t mimo_qam_slice(int32_t constel_size, const double* in_iq, int64_t n, int32_t* labels_out);
int32_t mimo_qam_llr(int32_t constel_size, const double* in_iq, int64_t n, const double* noise_var, double* llr_out);
int32_t mimo_qam_softbits(int32_t constel_size, const double* in_iq, int64_t n, double* out);
/* The coded mode's decoder on caller-given channel values (see mimo_engine_coded_points): chan is
 * [n_cw][N] int8, app_out [n_cw][N] int16 the final L of every bit.  chan may hold any integer with
 * |c| <= 63, 0 and even values included; beyond that, or for a code that breaks its rules,
 * MIMO_EINVAL before any HIP call.  n_cw = 0 is MIMO_OK with nothing read or written. */
int32_t mimo_ldpc_decode(const mimo_ldpc_code* code, const int8_t* chan, int64_t n_cw, int16_t* app_out);
int32_t mimo_fft(int32_t n_fft, int64_t batch, int32_t inverse, const double* in_iq, double* out_iq);
int32_t mimo_ofdm_tx(int32_t n_fft, int32_t n_sub_carr, int32_t cp_len, int64_t batch, const double* sym_iq,
                     double* td_iq);
int32_t mimo_ofdm_rx(int32_t n_fft, int32_t n_sub_carr, int32_t cp_len, int64_t batch, const double* td_iq,
                     double* sym_iq);
int32_t mimo_pa(int32_t kind, double sat_pow, double p_hardness, double toi_coeff, const double* in_iq, int64_t n,
                double* out_iq);
/* Bussgang gain alpha(IBO) for n IBO values [dB], by the trial kernel's segment table
 * (alpha_fit.h: the float64 kernels' alpha for antennas outside the per-point fit).  (ABI 6) */
int32_t mimo_calc_alpha(const double* ibo_db, int64_t n, double* out);
int32_t mimo_mrt_precode(int32_t n_ant, int32_t n_cols, const double* h_iq, double* p_iq);
int32_t mimo_combine(int32_t n_ant, int64_t n, const double* h_iq, const double* y_iq, double* out_iq);
int32_t mimo_awgn(uint64_t seed, uint64_t counter, int64_t n, double noise_std, const double* in_iq, double* out_iq);
int32_t mimo_count_bit_errors(const int64_t* a, const int64_t* b, int64_t n, int64_t* out);
int32_t mimo_cnc_receive(int32_t constel_size, int32_t n_fft, int32_t n_sub_carr, int32_t pa_kind, double sat_pow,
                         double p_hardness, double toi_coeff, double alpha, const int32_t* iters, int32_t n_iters,
                         const double* in_sc_iq, int32_t* labels_out);
/* ABI 7: the same loop with optional outputs -- labels_out [n_iters][S] and/or
 * corrected_iq_out [n_iters][S] (re, im), the slicer input rx - d of each listed iteration,
 * which CncReceiver.receive(return_bits=False) returns (corrector.py:80-84).  Either may be
 * null. */
int32_t mimo_cnc_receive_ex(int32_t constel_size, int32_t n_fft, int32_t n_sub_carr, int32_t pa_kind, double sat_pow,
                            double p_hardness, double toi_coeff, double alpha, const int32_t* iters, int32_t n_iters,
                            const double* in_sc_iq, int32_t* labels_out, double* corrected_iq_out);

#ifdef __cplusplus
}
#endif
#endif /* MIMO_ENGINE_H */
