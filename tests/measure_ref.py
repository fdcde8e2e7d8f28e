"""Reference for the engine's measure mode (mimo_engine_measure_points), built from the oracle.

Per trial the row ``[Es, Ez0, Re C, Im C, Ed0, Ee_0 ...]`` over the S data sub-carriers:
``s`` the transmitted points, ``z`` / ``z0`` the AGC'd received vector with the trial's noise /
with ``z_noise = 0`` (two ``oracle.sim.run_trial(..., return_debug=True)`` calls), ``v_i`` the
slicer input of counter index i -- ``refmath.cnc_receive(..., return_bits=False)`` for CNC, a
restatement of ``sim.mcnc_receive`` that keeps ``v`` for MCNC, and ``z_c`` of ``run_trial``'s
clean branch for the clean index.  Also ``Ez = sum |z|^2``, which scales the tests' bounds.
"""
import numpy as np

from oracle import refmath as rm
from oracle import sim

MEAS_FIXED = 5


def mcnc_slicer_inputs(cfg, iters, z, const, p, h_prop, agc_vec, pp, gain):
    """``sim.mcnc_receive`` (corrector.py:165-207), returning {iteration: slicer input v}."""
    out = {}
    d = None
    for it in range(max(iters) + 1):
        v = z if it == 0 else z - d
        s_hat = const[rm.detect_labels(const, v)]
        if it in iters:
            out[it] = v
        y = sim._tx_pa(cfg, s_hat[None, :] * p, pp, gain)
        d = np.sum(h_prop * y, axis=0) / agc_vec - s_hat
    return out


def trial_row(cfg, d, j, iters, incl_clean):
    """(counts, row, Ez) of trial j of the draws ``d`` (``sim.draws``)."""
    iters = sorted(set(int(i) for i in iters))
    pp = sim.point_params(cfg)
    const = pp["const"]
    labels = d["labels"][j]
    z_csi = d["z_csi"][j] if "z_csi" in d else None
    counts, dbg = sim.run_trial(cfg, labels, d["z_chan"][j], d["z_noise"][j], d["loc_u"][j], z_csi, iters,
                                incl_clean, return_debug=True)
    _, dbg0 = sim.run_trial(cfg, labels, d["z_chan"][j], np.zeros_like(d["z_noise"][j]), d["loc_u"][j], z_csi,
                            iters, incl_clean, return_debug=True)
    s = const[labels]
    z, z0 = dbg["z"], dbg0["z"]
    g = dbg["agc"]
    v = []
    if incl_clean:
        # run_trial's clean branch (mp_model.py:159-169)
        r_c = np.sum(dbg["h"] * (s[None, :] * dbg["p"]), axis=0)
        n_c = np.sqrt(pp["es"] * g["hk_vk_noise"] / pp["snr"]) * d["z_noise"][j]
        v.append((r_c + n_c) / g["hk_vk"])
    if cfg.receiver == "cnc":
        vi = rm.cnc_receive(iters, z, const, cfg.n_fft, pp["cnc_pa"], pp["cnc_sat"], cfg.p_hardness,
                            pp["cnc_coeff"], pp["cnc_alpha"], return_bits=False)
    else:
        h_est = rm.csi_error(dbg["h"], cfg.csi_eps, z_csi) if cfg.csi_eps is not None else dbg["h"]
        vi = mcnc_slicer_inputs(cfg, iters, z, const, dbg["p"], h_est, g["ak_hk_vk"], pp, dbg["gain"])
    v.extend(vi[i] for i in iters)
    c = np.sum(z0 * np.conj(s))
    row = [np.sum(np.abs(s) ** 2), np.sum(np.abs(z0) ** 2), c.real, c.imag, np.sum(np.abs(z0 - s) ** 2)]
    row.extend(np.sum(np.abs(vv - s) ** 2) for vv in v)
    return np.asarray(counts, np.int64), np.asarray(row, np.float64), float(np.sum(np.abs(z) ** 2))


def reference_rows(cfg, seed, trials, iters, incl_clean=False, chunk=8):
    """-> (counts [n, n_idx] int64, rows [n, MEAS_FIXED + n_idx] float64, Ez [n])."""
    trials = np.asarray(trials, dtype=np.int64)
    counts, rows, ez = [], [], []
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            c, r, e = trial_row(cfg, d, j, iters, incl_clean)
            counts.append(c)
            rows.append(r)
            ez.append(e)
    return np.asarray(counts), np.asarray(rows), np.asarray(ez)


EPS_Z = 1e-13  # relative l2 error allowed on z (see row_bounds)


def row_bounds(rows, ez):
    """Allowed |gpu - ref| per entry of the per-trial rows.  With eps = 1e-13 the relative l2
    error allowed on z -- ten times the 1e-14 tests/test_gpu_probe_fft.py allows one float64
    IFFT -> PA -> FFT chain, the factor covering the antenna sum and the AGC divide -- a column
    X = sum |a - b|^2 whose ``a`` carries that error moves by at most
    2 eps sqrt(X Ez) + 1e-12 X; Es, Ez0 and C by 1e-12 Ez."""
    rows = np.asarray(rows, np.float64)
    ez = np.asarray(ez, np.float64)[:, None]
    b = 2 * EPS_Z * np.sqrt(np.abs(rows) * ez) + 1e-12 * np.abs(rows)
    b[:, :4] = 1e-12 * ez
    return b
