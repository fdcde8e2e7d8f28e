"""Reference for the engine's soft mode (mimo_engine_soft_points), built from the oracle.

Per trial and counter index the histogram of the ``S log2 M`` bit reliabilities of the slicer input
``v_i`` that index slices, obtained the way ``measure_ref`` obtains it: ``z_c`` of ``run_trial``'s
clean branch, ``refmath.cnc_receive(..., return_bits=False)`` for CNC,
``measure_ref.mcnc_slicer_inputs`` for MCNC.  The metric is include/mimo_engine.h's, by brute force
over the L levels of an axis: ``lambda = (d0 - d1) (d0 + d1) 0.25`` with ``d_b`` the distance to the
nearest level whose Gray bit is b, each step one IEEE double operation (numpy never fuses them).
"""
import numpy as np

import envelope_ref
import measure_ref
from oracle import refmath as rm
from oracle import sim

SOFT_BINS = 256
EPS_V = 1e-11  # envelope_ref.EPS_X's argument: relative error of a sample, in units of the largest
assert EPS_V == envelope_ref.EPS_X


def axis_tables(constel_size):
    """(levels [L], gray bit of every level [hb, L] with row 0 the MSB)."""
    L = int(round(np.sqrt(constel_size)))
    hb = int(round(np.log2(L)))
    idx = np.arange(L)
    gray = idx ^ (idx >> 1)
    bits = np.stack([(gray >> j) & 1 for j in range(hb - 1, -1, -1)])
    return np.arange(-L + 1, L, 2).astype(np.float64), bits.astype(bool)


def axis_lambda(constel_size, x):
    """Brute-force lambda of real coordinates ``x`` [n] -> [n, hb], MSB first."""
    levels, bits = axis_tables(constel_size)
    x = np.asarray(x, np.float64).reshape(-1)
    d = np.abs(x[:, None] - levels[None, :])
    out = np.empty((x.size, bits.shape[0]))
    for r, one in enumerate(bits):
        d0, d1 = d[:, ~one].min(axis=1), d[:, one].min(axis=1)
        out[:, r] = (d0 - d1) * (d0 + d1) * 0.25
    return out


def lam(constel_size, v):
    """lambda of complex slicer inputs ``v`` [n] -> [n, log2 M]: the I-axis bits MSB first, then Q."""
    v = np.asarray(v, np.complex128).reshape(-1)
    return np.concatenate([axis_lambda(constel_size, v.real), axis_lambda(constel_size, v.imag)], axis=1)


def label_bits(constel_size, labels):
    """The transmitted bits [n, log2 M], MSB first: the layout of ``lam``."""
    nb = int(round(np.log2(constel_size)))
    return rm.labels_to_bits(labels, nb).reshape(-1, nb).astype(bool)


def rho(constel_size, v, labels):
    """Reliabilities [n, log2 M]: lambda where the transmitted bit is 1, -lambda where it is 0."""
    la = lam(constel_size, v)
    return np.where(label_bits(constel_size, labels), la, -la)


def bin_of(r, rho_max):
    """clamp(floor(rho * scale), -128, 127) + 128 with scale = 128.0 / rho_max, the clamp in double."""
    scale = np.float64(128.0) / np.float64(rho_max)
    f = np.floor(np.asarray(r, np.float64) * scale)
    return (np.clip(f, -128.0, 127.0)).astype(np.int64) + 128


def row_of(constel_size, vs, labels, rho_max):
    """Row [n_idx, 256] of a trial whose counter indices slice ``vs`` (a list of [S] vectors)."""
    return np.stack([np.bincount(bin_of(rho(constel_size, v, labels), rho_max).ravel(), minlength=SOFT_BINS)
                     for v in vs]).astype(np.float64)


def near_edge(constel_size, v, labels, rho_max):
    """Number of reliabilities of ``v`` that an error of ``delta = L EPS_V max_k |v_k|`` could move
    across a bin edge (|d lambda / dx| = (d0 + d1) / 2 on the nearer side stays below L, so a
    coordinate error of EPS_V max |v| moves rho by less than delta)."""
    L = np.sqrt(constel_size)
    r = rho(constel_size, v, labels)
    delta = L * EPS_V * np.abs(np.asarray(v)).max()
    return int(np.count_nonzero(bin_of(r - delta, rho_max) != bin_of(r + delta, rho_max)))


def zeros(constel_size, v, labels):
    """Number of reliabilities that are exactly 0 (a coordinate on a decision boundary)."""
    return int(np.count_nonzero(rho(constel_size, v, labels) == 0))


def slicer_inputs(cfg, d, j, iters, incl_clean):
    """(counts, labels, [v_i per counter index]) of trial j of the draws ``d`` (``sim.draws``); the
    vectors as ``measure_ref.trial_row`` obtains them."""
    iters = sorted(set(int(i) for i in iters))
    pp = sim.point_params(cfg)
    const = pp["const"]
    labels = d["labels"][j]
    z_csi = d["z_csi"][j] if "z_csi" in d else None
    counts, dbg = sim.run_trial(cfg, labels, d["z_chan"][j], d["z_noise"][j], d["loc_u"][j], z_csi, iters,
                                incl_clean, return_debug=True)
    s = const[labels]
    z, g = dbg["z"], dbg["agc"]
    v = []
    if incl_clean:
        r_c = np.sum(dbg["h"] * (s[None, :] * dbg["p"]), axis=0)
        n_c = np.sqrt(pp["es"] * g["hk_vk_noise"] / pp["snr"]) * d["z_noise"][j]
        v.append((r_c + n_c) / g["hk_vk"])
    if cfg.receiver == "cnc":
        vi = rm.cnc_receive(iters, z, const, cfg.n_fft, pp["cnc_pa"], pp["cnc_sat"], cfg.p_hardness,
                            pp["cnc_coeff"], pp["cnc_alpha"], return_bits=False)
    else:
        h_est = rm.csi_error(dbg["h"], cfg.csi_eps, z_csi) if cfg.csi_eps is not None else dbg["h"]
        vi = measure_ref.mcnc_slicer_inputs(cfg, iters, z, const, dbg["p"], h_est, g["ak_hk_vk"], pp, dbg["gain"])
    v.extend(vi[i] for i in iters)
    return np.asarray(counts, np.int64), labels, v


def reference(cfg, seed, trials, iters, rho_max, incl_clean=False, chunk=8):
    """-> (counts [n, n_idx] int64, rows [n, n_idx, 256] float64, near-edge count, exact zeros)."""
    trials = np.asarray(trials, dtype=np.int64)
    M = cfg.constel_size
    counts, rows, near, nz = [], [], 0, 0
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            c, labels, vs = slicer_inputs(cfg, d, j, iters, incl_clean)
            counts.append(c)
            rows.append(row_of(M, vs, labels, rho_max))
            near += sum(near_edge(M, v, labels, rho_max) for v in vs)
            nz += sum(zeros(M, v, labels) for v in vs)
    return np.asarray(counts), np.asarray(rows), near, nz
