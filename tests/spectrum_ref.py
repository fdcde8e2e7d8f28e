"""Reference for the engine's spectrum mode (mimo_engine_spectrum_points), built from the oracle.

Per trial the row ``[psd[0] ... psd[F-1], Ex, Re C, Im C]``: ``x = s p`` the precoded input of
every antenna (``p`` and the precoding ``gain`` from ``oracle.sim.run_trial(..., return_debug=True)``;
with a CSI error ``p`` comes from the estimate), ``Y = FFT(PA(IFFT(x)))`` on all F bins --
``sim._tx_pa`` restated without its final ``[:, bins]`` -- then ``psd = sum_a |Y_a|^2`` in
``numpy.fft`` bin order, ``Ex = sum |x|^2`` and ``C = sum Y[:, bins] conj(x)``.
"""
import numpy as np

from oracle import refmath as rm
from oracle import sim

SPEC_FIXED = 3


def tx_pa_full(cfg, x_sc, pp, gain):
    """``sim._tx_pa`` keeping every FFT bin: [A, S] -> [A, F]."""
    bins = rm.inband_bins(cfg.n_fft, cfg.n_sc)
    fd = np.zeros((x_sc.shape[0], cfg.n_fft), dtype=np.complex128)
    fd[:, bins] = x_sc
    td = np.fft.ifft(fd, norm="ortho", axis=-1)
    avg = pp["avg_samp"] * gain  # AntennaArray.update_distortion (antenna_array.py:337-360)
    if cfg.pa == "toi":
        td = rm.toi(rm.toi_coeff(cfg.ibo_db, avg), td)
    elif cfg.pa != "none":
        td = rm.apply_pa(cfg.pa, td, rm.sat_pow(cfg.ibo_db, avg), cfg.p_hardness)
    return np.fft.fft(td, norm="ortho", axis=-1)


def trial_row(cfg, d, j, iters, incl_clean):
    """(counts, row) of trial j of the draws ``d`` (``sim.draws``)."""
    iters = sorted(set(int(i) for i in iters))
    pp = sim.point_params(cfg)
    labels = d["labels"][j]
    z_csi = d["z_csi"][j] if "z_csi" in d else None
    counts, dbg = sim.run_trial(cfg, labels, d["z_chan"][j], d["z_noise"][j], d["loc_u"][j], z_csi, iters,
                                incl_clean, return_debug=True)
    x = pp["const"][labels][None, :] * dbg["p"]
    y = tx_pa_full(cfg, x, pp, dbg["gain"])
    c = np.sum(y[:, rm.inband_bins(cfg.n_fft, cfg.n_sc)] * np.conj(x))
    row = np.concatenate([(np.abs(y) ** 2).sum(0), [np.sum(np.abs(x) ** 2), c.real, c.imag]])
    return np.asarray(counts, np.int64), row


def reference_rows(cfg, seed, trials, iters, incl_clean=False, chunk=8):
    """-> (counts [n, n_idx] int64, rows [n, F + SPEC_FIXED] float64)."""
    trials = np.asarray(trials, dtype=np.int64)
    counts, rows = [], []
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            c, r = trial_row(cfg, d, j, iters, incl_clean)
            counts.append(c)
            rows.append(r)
    return np.asarray(counts), np.asarray(rows)


EPS_Y = 1e-13  # relative l2 error allowed on a chain output Y_a (measure_ref.EPS_Z)


def row_bounds(rows):
    """Allowed |gpu - ref| per cell of the per-trial rows.  With Ptot = sum_k psd[k] and eps the
    relative l2 error allowed on every antenna's chain output (|dY_a| <= eps |Y_a|), Cauchy-Schwarz
    over the antennas moves psd[k] = sum_a |Y_a[k]|^2 by at most
    2 eps sqrt(psd[k] Ptot) + eps^2 Ptot (the second term keeps the bound positive where the
    reference is exactly 0), plus 1e-12 psd[k] for the sum itself; Ex and C by 1e-12 Ptot."""
    rows = np.asarray(rows, np.float64)
    psd = rows[:, :-SPEC_FIXED]
    ptot = psd.sum(1, keepdims=True)
    b = np.empty_like(rows)
    b[:, :-SPEC_FIXED] = 2 * EPS_Y * np.sqrt(psd * ptot) + EPS_Y ** 2 * ptot + 1e-12 * psd
    b[:, -SPEC_FIXED:] = 1e-12 * ptot
    return b
