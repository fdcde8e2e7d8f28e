"""Reference for the engine's envelope mode (mimo_engine_envelope_points), built from the oracle.

Per trial the row ``[hist_in[0..127], hist_out[0..127], Pin, Pout, Re C, Im C]``: ``X = s p`` the
precoded input of every antenna (``p`` and the precoding ``gain`` from
``oracle.sim.run_trial(..., return_debug=True)``; with a CSI error ``p`` comes from the estimate),
``x = IFFT(X)`` (ortho) the PA input of all F time samples, ``y = PA(x)`` (``rm.apply_pa`` /
``rm.toi`` as ``sim._tx_pa`` applies them), the two histograms of ``|x|^2`` and ``|y|^2`` over the
bins of include/mimo_engine.h -- computed on ``float64.view(uint64)`` -- and ``Pin = sum |x|^2``,
``Pout = sum |y|^2``, ``C = sum y conj(x)``.
"""
import numpy as np

from oracle import refmath as rm
from oracle import sim

ENV_BINS = 128
ENV_FIXED = 4
ENV_WIDTH = 2 * ENV_BINS + ENV_FIXED
BIN_BASE = (1023 - 12) << 3  # 8088

# Relative amplitude error allowed on a time sample, in units of its antenna's largest sample: the
# project's relative l2 bound on a chain, EPS_Y = 1e-13 (measure_ref.EPS_Z), times sqrt(8192) for
# the worst case of the whole l2 error in one sample of the largest transform, rounded up.
EPS_X = 1e-11


def nominal_power(cfg):
    """The array's nominal mean sample power at a PA input: ``avg_samp / n_ant`` (MRT: mean |P|^2 = 1/A),
    the power ``sat_pow`` is formed from."""
    return sim.point_params(cfg)["avg_samp"] / cfg.n_ant


def power(z):
    """re re + im im, as the header states pw."""
    z = np.asarray(z, np.complex128)
    return z.real * z.real + z.imag * z.imag


def bin_of(pw, ref_pow):
    """The bin of sample powers ``pw``: clamp((bits(pw scale) >> 49) - 8088, 0, 127)."""
    scale = np.float64(1.0625) / np.float64(ref_pow)
    v = np.ascontiguousarray(np.asarray(pw, np.float64) * scale)
    b = (v.view(np.uint64) >> np.uint64(49)).astype(np.int64) - BIN_BASE
    return np.clip(b, 0, ENV_BINS - 1)


def edges():
    """Lower edges of bins 1 ... 127 in units of u = |.|^2 / ref_pow, by the header's formula."""
    b = np.arange(1, ENV_BINS)
    return 2.0 ** (-12 + b // 8) * (1 + (b % 8) / 8) * 16 / 17


def trial_samples(cfg, d, j, iters, incl_clean=False):
    """(counts, x [A, F], y [A, F]) of trial j of the draws ``d`` (``sim.draws``)."""
    iters = sorted(set(int(i) for i in iters))
    pp = sim.point_params(cfg)
    labels = d["labels"][j]
    z_csi = d["z_csi"][j] if "z_csi" in d else None
    counts, dbg = sim.run_trial(cfg, labels, d["z_chan"][j], d["z_noise"][j], d["loc_u"][j], z_csi, iters,
                                incl_clean, return_debug=True)
    fd = np.zeros((cfg.n_ant, cfg.n_fft), dtype=np.complex128)
    fd[:, rm.inband_bins(cfg.n_fft, cfg.n_sc)] = pp["const"][labels][None, :] * dbg["p"]
    x = np.fft.ifft(fd, norm="ortho", axis=-1)
    avg = pp["avg_samp"] * dbg["gain"]  # AntennaArray.update_distortion (antenna_array.py:337-360)
    if cfg.pa == "toi":
        y = rm.toi(rm.toi_coeff(cfg.ibo_db, avg), x)
    elif cfg.pa != "none":
        y = rm.apply_pa(cfg.pa, x, rm.sat_pow(cfg.ibo_db, avg), cfg.p_hardness)
    else:
        y = x.copy()
    return np.asarray(counts, np.int64), x, y


def row_of(x, y, ref_pow):
    pin, pout = power(x), power(y)
    c = np.sum(y * np.conj(x))
    return np.concatenate([np.bincount(bin_of(pin, ref_pow).ravel(), minlength=ENV_BINS),
                           np.bincount(bin_of(pout, ref_pow).ravel(), minlength=ENV_BINS),
                           [pin.sum(), pout.sum(), c.real, c.imag]]).astype(np.float64)


def movable(z, delta, ref_pow):
    """Number of samples of ``z`` [A, F] whose bin an amplitude error of ``delta`` [A, 1] could change."""
    r = np.abs(z)
    lo, hi = np.maximum(r - delta, 0.0), r + delta
    return int(np.count_nonzero(bin_of(lo * lo, ref_pow) != bin_of(hi * hi, ref_pow)))


def _trials(cfg, seed, trials, iters, incl_clean, chunk):
    trials = np.asarray(trials, dtype=np.int64)
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            yield trial_samples(cfg, d, j, iters, incl_clean)


def reference(cfg, seed, trials, iters, ref_pow, incl_clean=False, chunk=8):
    """-> (counts [n, n_idx] int64, rows [n, 260] float64, near-edge sample count): one pass of the
    oracle for ``reference_rows`` and ``near_edge``."""
    counts, rows, near = [], [], 0
    for c, x, y in _trials(cfg, seed, trials, iters, incl_clean, chunk):
        counts.append(c)
        rows.append(row_of(x, y, ref_pow))
        delta = EPS_X * np.abs(x).max(axis=1, keepdims=True)
        near += movable(x, delta, ref_pow) + movable(y, delta, ref_pow)
    return np.asarray(counts), np.asarray(rows), near


def reference_rows(cfg, seed, trials, iters, ref_pow, incl_clean=False, chunk=8):
    """-> (counts [n, n_idx] int64, rows [n, 260] float64)."""
    counts, rows, _ = reference(cfg, seed, trials, iters, ref_pow, incl_clean, chunk)
    return counts, rows


def near_edge(cfg, seed, trials, iters, ref_pow, chunk=8):
    """The number of samples, PA inputs and outputs, that an amplitude error of
    ``EPS_X * max_n |x_a[n]|`` could move across a bin edge."""
    return reference(cfg, seed, trials, iters, ref_pow, False, chunk)[2]
