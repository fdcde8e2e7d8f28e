"""Reference for the engine's beam mode (mimo_engine_beam_points), built from the oracle.

Per trial and probe position q the row ``[Py_in, Py_oob, Px, Re C, Im C]``: ``x = s p`` the precoded
input of every antenna and ``y = FFT(PA(IFFT(x)))`` on all F bins as in ``tests/spectrum_ref.py``,
``G_q = oracle.refmath.los_channel`` from the array to the probe (all F bins, gain 0 dB), the field
``R_q[k] = sum_a G_q[a,k] y_a[k]`` and its linear part's source ``U_q[k] = sum_a G_q[a,k] x_a[k]``
(in band), then ``Py_in = sum_band |R|^2``, ``Py_oob = sum_offband |R|^2``, ``Px = sum_band |U|^2``
and ``C = sum_band R conj(U)``.
"""
import functools
import math

import numpy as np

import spectrum_ref
from oracle import refmath as rm
from oracle import sim

BEAM_FIXED = 5
EPS_Y = spectrum_ref.EPS_Y  # relative l2 error allowed on a chain output Y_a (and on its input X_a)
EPS_SUM = 1e-12             # relative rounding allowed on a sum of up to A F non-negative terms


def probe_channels(cfg, probes):
    """[n_probes, A, F]: the LoS channel from every antenna to every probe position."""
    return np.stack([rm.los_channel(cfg.tx_pos, np.asarray(q, np.float64), cfg.n_fft, cfg.carrier_spacing,
                                    cfg.center_freq) for q in np.asarray(probes, np.float64).reshape(-1, 3)])


def eps_g(cfg, probes):
    """Relative error allowed on each entry of G: 2 pi 8 2^-53 max(d f / c) + 4 2^-53.

    The phase 2 pi d f / c is of the order of 2 pi 3500 rad here, so a relative rounding of 2^-53 in
    its argument moves it by 2 pi (d f / c) 2^-53 rad.  Eight such roundings are allowed, the
    reference's and the device's together.  The reference (``los_channel``): the sum and the square
    root of d (2), the product d f (1), the factor 2 pi (pi as a double, and the product: 2), the
    division by c (1) -- six.  The device forms the phase in cycles from the same d: f / c (1) and
    d (f / c) (1) -- two; its reduction u - rint(u) is exact.  The second term covers the four
    roundings of the amplitude c / (4 pi d f) and the final sin / cos."""
    tx = np.asarray(cfg.tx_pos, np.float64)
    pr = np.asarray(probes, np.float64).reshape(-1, 3)
    d = np.sqrt(((tx[None, :, :] - pr[:, None, :]) ** 2).sum(-1))
    f = rm.fftfreq_carriers(cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)
    u = d.max() * f.max() / rm.SPEED_OF_LIGHT
    return 2 * np.pi * 8 * 2.0 ** -53 * u + 4 * 2.0 ** -53


def sums_of(x, y, g, n_fft, n_sc):
    """The five sums for every probe: x [A, S], y [A, F], g [n_probes, A, F] -> [n_probes, 5]."""
    bins = rm.inband_bins(n_fft, n_sc)
    off = np.ones(n_fft, bool)
    off[bins] = False
    r = np.einsum("qak,ak->qk", g, y)
    u = np.einsum("qak,ak->qk", g[:, :, bins], x)
    c = np.sum(r[:, bins] * np.conj(u), axis=1)
    return np.stack([(np.abs(r[:, bins]) ** 2).sum(1), (np.abs(r[:, off]) ** 2).sum(1), (np.abs(u) ** 2).sum(1),
                     c.real, c.imag], axis=1)


def row_bounds(x, y, g, n_fft, n_sc, eg):
    """Allowed |gpu - ref| per cell of one trial's rows, [n_probes, 5], from the inputs alone: every
    antenna's chain output and input may be off by eps_Y in relative l2 norm over the bins
    (|dY_a| <= eps_Y |Y_a|, the same for X_a) and every G entry by eps_G relative.

    With M[k] = sum_a |G[a,k]| |Y_a[k]|, g2 = max_k sum_a |G[a,k]|^2 and Ptot = sum_a |Y_a|^2,
    Cauchy-Schwarz over the antennas, then over the bins, bounds the l2 error of the field R over
    any set B of bins by  E_R(B) = eps_G |M|_B + (1 + eps_G) eps_Y sqrt(g2 Ptot)  (the error of a
    chain output may sit in any bins, so its term keeps the whole Ptot), and the same with X for U.
    Then  |d sum_B |R|^2| <= 2 |R|_B E_R(B) + E_R(B)^2,  and for C = sum_band R conj(U)
    |dC| <= |R|_band E_U + |U| E_R(band) + E_R(band) E_U.  The squared terms keep the bounds positive
    where the reference is exactly 0.  EPS_SUM times the sum of the terms' magnitudes is added for
    the roundings of the sums themselves (up to A F terms of 2^-53 each: 2e-12 at the largest case,
    of which a sum of non-negative terms realises a small part)."""
    bins = rm.inband_bins(n_fft, n_sc)
    off = np.ones(n_fft, bool)
    off[bins] = False
    ag = np.abs(g)
    r = np.einsum("qak,ak->qk", g, y)
    u = np.einsum("qak,ak->qk", g[:, :, bins], x)
    m_y = np.einsum("qak,ak->qk", ag, np.abs(y))
    m_x = np.einsum("qak,ak->qk", ag[:, :, bins], np.abs(x))
    g2 = (ag ** 2).sum(1).max(1)
    g2_in = (ag[:, :, bins] ** 2).sum(1).max(1)
    ptot, pxtot = (np.abs(y) ** 2).sum(), (np.abs(x) ** 2).sum()
    l2 = lambda a: np.sqrt((np.abs(a) ** 2).sum(1))  # noqa: E731
    e_chain = (1 + eg) * EPS_Y * np.sqrt(g2 * ptot)
    e_in, e_off = eg * l2(m_y[:, bins]) + e_chain, eg * l2(m_y[:, off]) + e_chain
    e_u = eg * l2(m_x) + (1 + eg) * EPS_Y * np.sqrt(g2_in * pxtot)
    r_in, r_off, u_n = l2(r[:, bins]), l2(r[:, off]), l2(u)
    b = np.empty((g.shape[0], BEAM_FIXED))
    b[:, 0] = 2 * r_in * e_in + e_in ** 2 + EPS_SUM * r_in ** 2
    b[:, 1] = 2 * r_off * e_off + e_off ** 2 + EPS_SUM * r_off ** 2
    b[:, 2] = 2 * u_n * e_u + e_u ** 2 + EPS_SUM * u_n ** 2
    b[:, 3] = b[:, 4] = r_in * e_u + u_n * e_in + e_in * e_u + EPS_SUM * (np.abs(r[:, bins]) * np.abs(u)).sum(1)
    return b


def trial_xy(cfg, d, j, iters, incl_clean):
    """(counts, x [A, S], y [A, F]) of trial j of the draws ``d`` (``sim.draws``)."""
    iters = sorted(set(int(i) for i in iters))
    pp = sim.point_params(cfg)
    labels = d["labels"][j]
    z_csi = d["z_csi"][j] if "z_csi" in d else None
    counts, dbg = sim.run_trial(cfg, labels, d["z_chan"][j], d["z_noise"][j], d["loc_u"][j], z_csi, iters,
                                incl_clean, return_debug=True)
    x = pp["const"][labels][None, :] * dbg["p"]
    return np.asarray(counts, np.int64), x, spectrum_ref.tx_pa_full(cfg, x, pp, dbg["gain"])


def reference_rows(cfg, seed, trials, iters, probes, incl_clean=False, chunk=8, bounds=True):
    """-> (counts [n, n_idx] int64, rows [n, n_probes, 5], allowed deviations [n, n_probes, 5] or None)."""
    trials = np.asarray(trials, dtype=np.int64)
    g = probe_channels(cfg, probes)
    eg = eps_g(cfg, probes)
    counts, rows, bnd = [], [], []
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            c, x, y = trial_xy(cfg, d, j, iters, incl_clean)
            counts.append(c)
            rows.append(sums_of(x, y, g, cfg.n_fft, cfg.n_sc))
            if bounds:
                bnd.append(row_bounds(x, y, g, cfg.n_fft, cfg.n_sc, eg))
    return np.asarray(counts), np.asarray(rows), (np.asarray(bnd) if bounds else None)


# ---------------------------------------------------------------- the physics system of the tests
# LoS (or Rayleigh) with the fixed user, A 8, F 512, S 256, 64-QAM, soft limiter; 37 probes at
# 0 ... 180 degrees in 5-degree steps on the circle through the default user position, at its height
PHYS = dict(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", snr_db=25.0, reroll=False)
PHYS_SEED, PHYS_TRIALS = 7, 32
PHYS_ANGLES = np.arange(0.0, 181.0, 5.0)
USER = int(np.argmin(np.abs(PHYS_ANGLES - 45.0)))  # the probe at the user


def phys_probes():
    from utilities import circle_probes
    rx = sim.SimConfig(n_ant=1, n_sc=4, n_fft=128, constel_size=4).rx_pos
    return circle_probes(PHYS_ANGLES, math.hypot(rx[0], rx[1]), rx[2])


@functools.lru_cache(maxsize=None)
def pooled_reference(channel, ibo, pa="softlim"):
    """(config, per-trial rows [PHYS_TRIALS, 37, 5]) of the physics system; computed once, read-only."""
    cfg = sim.SimConfig(**dict(PHYS, channel=channel, ibo_db=ibo, pa=pa))
    _, rows, _ = reference_rows(cfg, PHYS_SEED, np.arange(PHYS_TRIALS), (0,), phys_probes(), bounds=False)
    rows.setflags(write=False)
    return cfg, rows
