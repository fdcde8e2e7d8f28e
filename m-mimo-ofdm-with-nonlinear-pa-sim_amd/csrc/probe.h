/* libmimo_probe: accuracy probes of the fused trial kernel's building blocks.
 *
 * Test-only entry points (not part of include/mimo_engine.h, no ABI promise): each runs the
 * production device code -- the instance's FFT (trial_kernel.h trial_fft_t), pa_block, the
 * float64 table-driven primitives of real.h -- built from the same headers and on the same
 * host-built tables (host_tables.h) as libmimo_engine, on caller-owned host arrays, so that
 * tests can compare values with a long-double reference (tests/probe_util.py).
 *
 * Conventions: complex arrays are interleaved (re, im) of the instance's type (prec:
 * 0 = float64, 1 = float32, as MIMO_PREC_*); functions return 0 or a negative MIMO_PROBE_E*
 * code, with a message from mimo_probe_last_error() (thread-local).
 */
#ifndef MIMO_PROBE_H
#define MIMO_PROBE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MIMO_PROBE_OK = 0, MIMO_PROBE_EINVAL = -1, MIMO_PROBE_EHIP = -2, MIMO_PROBE_ENOINST = -3 };

const char* mimo_probe_last_error(void);

/* FFT instances.  prec 0: variant 0 = trial_fft_t<double, F, team_size64(F), 1>.
 * prec 1: variant 0 / 1 = trial_fft_t<float, F, team_size(F), NBUF = 1 / 2>, variant 2 / 3 = the
 * same on alt_team_size(F) (only where it differs from team_size(F): MIMO_PROBE_ENOINST else).
 * F in {128, ..., 8192}. */

/* Team size, production zero mask (bit m: bins [T m, T (m + 1)) are zero in every thread with
 * the band S = F / 2; 0 where that band runs the generic slot map) and FFT kind (0 team,
 * 1 wave-split, 2 split) of an instance.  Host only. */
int32_t mimo_probe_fft_info(int32_t prec, int32_t F, int32_t variant, int32_t* team, uint32_t* zero_mask,
                            int32_t* fft_kind);

/* Per row (one workgroup): out = FFT(PA(IFFT(in))), both transforms un-normalised, exactly the
 * kernel's sequence run<+1, 0, ZM> -> pa_block -> run_second<-1>.  masked != 0: the registers of
 * the zero mask are cleared and the IFFT skips them (ZM = the mask); else ZM = 0.
 * pa_kind: MIMO_PA_* (0 none, 1 soft limiter, 2 Rapp, 3 third-order). */
int32_t mimo_probe_fft(int32_t prec, int32_t F, int32_t variant, int32_t masked, int32_t pa_kind, double sat, double p,
                       double toi, int32_t n_rows, const void* in_freq, void* out_freq);

/* float64 primitives, elementwise over n inputs, lut64 filled as the kernel fills it.
 *   fn 0: ln_unit<-32>(w + 0.5), in = uint32 words        -> out0
 *   fn 1: sincos_lut(w), in = uint32 words               -> out0 = sin, out1 = cos
 *   fn 2: sincos_rev_lut(r), in = doubles (revolutions)  -> out0 = sin, out1 = cos
 *   fn 3: sqrt_n1   fn 4: rsq_n1   fn 5: rsq_r(double)   fn 6: rpow_neg_inv<4>   fn 7: rpow_neg_inv<6>
 *         in = doubles -> out0
 * out1 may be null for the single-output functions. */
int32_t mimo_probe_math(int32_t fn, int64_t n, const void* in, double* out0, double* out1);

/* pa_block<cold_out != 0> on 8-element register tiles of n complex samples. */
int32_t mimo_probe_pa(int32_t prec, int32_t cold_out, int32_t pa_kind, double sat, double p, double toi, int64_t n,
                      const void* in_iq, void* out_iq);

/* Host only: the per-point Bussgang-gain fits (host_tables.h fit_alpha). */
int32_t mimo_probe_alpha_fit(double g0sq, double* amono19, double* apoly9, double* xlim);

/* Host only: a production table as complex pairs of the precision's type.  kind 0: the team
 * FFT's table of team_size64(F) / team_size(F) (stage twiddles, then the cot-tan region; F 8192
 * float64: the split FFT's, as the engine uploads it); 1: the float32 table of alt_team_size(F);
 * 2: the wave-split FFT's (float64, F where the instance uses it); 3: the split FFT's (float64,
 * F 8192); 4: lut64 (float64; F ignored).  *n in: capacity of buf in pairs (buf may be null);
 * out: the table's length.  Copies only if it fits. */
int32_t mimo_probe_table(int32_t kind, int32_t prec, int32_t F, void* buf, int64_t* n);

/* Host only: the transform addresses that the float64 wave-split instance at F (1024, 2048) holds
 * across its antenna loop (wave_fft.h XAddr).  words: [T][3] packed words (address pairs, low half
 * first: cross | row, x0r | x1w, tw | x1r), computed by the kernel's formulas, or copied from
 * words_in if that is not null.  sites: [T][MIMO_PROBE_XADDR_SITES] byte offsets as the kernel's
 * accessors unpack them from those words: 0 the cross-wave base, 1 the wave's row plus lane,
 * 2 exchange 0's read base, 3 exchange 1's write base, 4 its read base, 5 / 6 the lane's offset in
 * the rows of stage 1's / stage 2's LDS constants, 7 / 8 the inverse's inter-step twiddle offsets
 * for k = 1 / 2, 9 the forward's.  info: T, waves, points per thread, butterflies NB, FW, row
 * elements, exchange array elements, R0, XS0, NS of stages 1 and 2, their offsets in the LDS
 * constants, that copy's entries, the inter-step twiddles' offset in the table, bytes per element,
 * constant rows of stages 1 and 2, exchange 1's padding shift, the table's entries, 1 where the
 * sub-transform's stages are in cot-tan form.  Without it (two-wave teams) stage 1's rows are its
 * twiddle block in the LDS copy and stage 2's are that stage's block of the table in global
 * memory, whose offset and rows the info then gives. */
#define MIMO_PROBE_XADDR_SITES 10
#define MIMO_PROBE_XADDR_INFO 21
int32_t mimo_probe_xaddr(int32_t F, const uint32_t* words_in, uint32_t* words, uint32_t* sites, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif
