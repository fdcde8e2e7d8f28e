"""CPU reference of the ray-cluster channel (include/mimo_engine.h, mimo_rays): the ray gains from
the oracle's Philox, the taps as long-double sums over the rays, the frequency response by
tdl_ref.ld_response.

    ray r in trial i under the key seed:
      (w0, w1, ., .) = Philox4x32-10 of counter (r, i mod 2^32, 8, 0)
      u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32
      diffuse:  c_r = ray_amp[r] sqrt(-ln u1) exp(j 2 pi u2);  specular:  c_r = ray_amp[r] exp(j 2 pi u2)
    g[a][l] = sum over the rays r of tap l of c_r steer[a][r]
    H[a][n] = sum_l g[a][l] exp(-j 2 pi n delays[l] / n_fft)
"""
import numpy as np

import probe_util as pu
import tdl_ref
from oracle import philox as px

LD, CLD = pu.LD, pu.CLD
STREAM_RAYS = 8


def ray_words(seed, trials, n_rays):
    """(w0, w1) uint32 [n, R] of the rays' counters; trials are taken mod 2^32."""
    t = (np.asarray(trials, dtype=object) % (1 << 32)).astype(np.uint64).reshape(-1, 1)
    r = np.arange(n_rays, dtype=np.uint64).reshape(1, -1)
    w0, w1, _, _ = px.philox4x32_10(r, t, STREAM_RAYS, np.zeros_like(r), int(seed) & 0xFFFFFFFFFFFFFFFF)
    return w0, w1


def _kinds(ray_amp, ray_kind):
    return np.zeros(len(ray_amp), bool) if ray_kind is None else np.asarray(ray_kind).astype(bool)


def np_gains(ray_amp, seed, trials, ray_kind=None):
    """The gains [n, R] in float64 by the oracle's box_muller's own steps: the yardstick."""
    w0, w1 = ray_words(seed, trials, len(ray_amp))
    u1 = (w0.astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = w1.astype(np.float64) * 2.0 ** -32
    rho = np.where(_kinds(ray_amp, ray_kind)[None, :], 1.0, np.sqrt(-np.log(u1))) * np.asarray(ray_amp, np.float64)[None, :]
    ang = 2.0 * np.pi * u2
    return rho * np.cos(ang) + 1j * rho * np.sin(ang)


def ld_gains(ray_amp, seed, trials, ray_kind=None):
    """The same in long double (the path of tdl_ref.ld_taps)."""
    w0, w1 = ray_words(seed, trials, len(ray_amp))
    u1 = (w0.astype(LD) + LD(0.5)) * LD(2.0 ** -32)
    u2 = w1.astype(LD) * LD(2.0 ** -32)
    rho = np.where(_kinds(ray_amp, ray_kind)[None, :], LD(1), np.sqrt(-np.log(u1))) * np.asarray(ray_amp, LD)[None, :]
    ang = 2 * pu.LD_PI * u2
    return rho * np.cos(ang) + CLD(1j) * (rho * np.sin(ang))


def ld_taps_of(gains, ray_tap, steer):
    """Taps [n, A, L] of gains [n, R] and steer [A, R] in long double: tap l sums its own rays."""
    g = np.asarray(gains, CLD)
    s = np.asarray(steer, CLD)
    rt = np.asarray(ray_tap, np.int64)
    onehot = (rt[:, None] == np.arange(rt.max() + 1)[None, :]).astype(LD)  # [R, L]
    return np.einsum("nr,ar,rl->nal", g, s, onehot)


def rays_channels(delays, ray_tap, ray_amp, steer, n_fft, seed, first_trial, n, ray_kind=None, taps=False, gains=False):
    """_engine.rays_channels on the CPU (float64 out): what the host tests put in its place."""
    trials = [int(first_trial) + j for j in range(int(n))]
    c = ld_gains(ray_amp, seed, trials, ray_kind)
    g = ld_taps_of(c, ray_tap, steer)
    h = tdl_ref.ld_response(g, delays, n_fft).astype(np.complex128)
    out = (h,) + ((g.astype(np.complex128),) if taps else ()) + ((c.astype(np.complex128),) if gains else ())
    return out if len(out) > 1 else h
