"""CPU reference of the tapped-delay-line channel (include/mimo_engine.h, mimo_tdl): the taps from
the oracle's Philox and Box-Muller, the frequency response as a direct DFT in long double.

    tap l of antenna a in trial i under the key seed:
      (w0, w1, ., .) = Philox4x32-10 of counter (l, i mod 2^32, 7, a)
      g = ant_amp[a] sqrt(powers[l]) sqrt(-ln u1) exp(j 2 pi u2),  u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32
    H[a][n] = sum_l g[a][l] exp(-j 2 pi n delays[l] / n_fft)
"""
import numpy as np

import probe_util as pu
from oracle import philox as px

LD, CLD = pu.LD, pu.CLD
STREAM_TDL = 7


def tap_words(seed, trials, n_ant, n_taps):
    """(w0, w1) uint32 [n, n_ant, L] of the taps' counters; trials are taken mod 2^32."""
    t = (np.asarray(trials, dtype=object) % (1 << 32)).astype(np.uint64).reshape(-1, 1, 1)
    a = np.arange(n_ant, dtype=np.uint64).reshape(1, -1, 1)
    tap = np.arange(n_taps, dtype=np.uint64).reshape(1, 1, -1)
    w0, w1, _, _ = px.philox4x32_10(tap, t, STREAM_TDL, a, int(seed) & 0xFFFFFFFFFFFFFFFF)
    return w0, w1


def _scale(powers, n_ant, ant_amp, dtype):
    amp = np.ones(n_ant, dtype) if ant_amp is None else np.asarray(ant_amp, dtype).reshape(-1)
    return amp[None, :, None] * np.sqrt(np.asarray(powers, dtype))[None, None, :]


def np_taps(powers, n_ant, seed, trials, ant_amp=None):
    """The taps [n, n_ant, L] in float64 by the oracle's box_muller: the yardstick."""
    w0, w1 = tap_words(seed, trials, n_ant, len(powers))
    return px.box_muller(w0, w1) * _scale(powers, n_ant, ant_amp, np.float64)


def ld_taps(powers, n_ant, seed, trials, ant_amp=None):
    """The same in long double (the path of stage_ref.ld_awgn_noise)."""
    w0, w1 = tap_words(seed, trials, n_ant, len(powers))
    u1 = (w0.astype(LD) + LD(0.5)) * LD(2.0 ** -32)
    u2 = w1.astype(LD) * LD(2.0 ** -32)
    rho = np.sqrt(-np.log(u1))
    ang = 2 * pu.LD_PI * u2
    return (rho * np.cos(ang) + CLD(1j) * (rho * np.sin(ang))) * _scale(powers, n_ant, ant_amp, LD)


def ld_response(taps, delays, n_fft):
    """H [..., n_fft] of taps [..., L]: the direct DFT in long double, the phase index n d reduced mod
    n_fft in integers first."""
    taps = np.asarray(taps, CLD)
    d = np.asarray(delays, np.int64)
    m = (np.arange(n_fft, dtype=np.int64)[:, None] * d[None, :]) % n_fft  # [F, L]
    ang = -2 * pu.LD_PI * m.astype(LD) / LD(n_fft)
    w = np.cos(ang) + CLD(1j) * np.sin(ang)
    return np.einsum("...l,nl->...n", taps, w)


def tdl_channels(delays, powers, n_ant, n_fft, seed, first_trial, n, ant_amp=None, taps=False):
    """_engine.tdl_channels on the CPU (float64 out): what the host tests put in its place."""
    trials = [int(first_trial) + j for j in range(int(n))]
    g = ld_taps(powers, n_ant, seed, trials, ant_amp)
    h = ld_response(g, delays, n_fft).astype(np.complex128)
    return (h, g.astype(np.complex128)) if taps else h
