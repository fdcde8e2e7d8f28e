"""Reference for the engine's turbo mode (mimo_engine_turbo_points, mimo_engine_cnc_step): the
definition next to ``mimo_engine_turbo_points`` in include/mimo_engine.h, built from the oracle's
received vector ``z`` (``sim.run_trial(..., return_debug=True)["z"]``), the soft mode's metric
(``soft_ref``), the coded mode's quantiser, interleaving and decoder (``ldpc_ref``) and the CNC step
of ``refmath.cnc_receive`` with the decided symbols in place of the slice.

Everything is integer after the quantiser's one ``floor``.
"""
import numpy as np

import ldpc_ref
import soft_ref
from oracle import refmath as rm
from oracle import sim


def cnc_step(cfg, pp, z, s_hat):
    """``z - dist`` with ``dist = FFT(PA_cnc(IFFT(up(s_hat)))) / alpha_cnc - s_hat`` (corrector.py:84-110,
    ``refmath.cnc_receive``'s loop body on given symbols)."""
    bins = rm.inband_bins(cfg.n_fft, z.shape[-1])
    up = np.zeros(cfg.n_fft, dtype=np.complex128)
    up[bins] = s_hat
    td = rm.apply_pa(pp["cnc_pa"], np.fft.ifft(up, norm="ortho"), pp["cnc_sat"], cfg.p_hardness, pp["cnc_coeff"])
    est = np.fft.fft(td, norm="ortho")[bins] / pp["cnc_alpha"]
    return z - (est - s_hat)


def decided_labels(cfg, code, labels, chan, L):
    """The decided labels of a pass: the transmitted bits XOR the decoder's decisions ``L < 0`` at the
    decoded positions and XOR the demapper's ``c < 0`` on the undecoded tail; bit j of sub-carrier k at
    stream position j S + k, MSB first (``rm.labels_to_bits``' layout)."""
    nb = int(round(np.log2(cfg.constel_size)))
    S = cfg.n_sc
    n_cw = chan.size // code.n_bits
    wrong = np.asarray(chan) < 0                                   # [stream]
    wrong[:n_cw * code.n_bits] = (np.asarray(L) < 0).T.reshape(-1)  # bit n of codeword w at n n_cw + w
    tx = rm.labels_to_bits(labels, nb).reshape(S, nb)              # [k, j]
    return rm.bits_to_labels((tx ^ wrong.reshape(nb, S).T.astype(np.int8)).reshape(-1), nb)


def trial(cfg, code, pp, labels, z, rho_max, n_passes, feedback="decoder"):
    """One trial -> (chan [n_passes, stream] int8, rows [n_passes, 4], v [n_passes, S], near, zeros).
    ``feedback="hard"`` feeds the hard slices back instead (the fused CNC loop)."""
    M, const = cfg.constel_size, pp["const"]
    chans, rows, vs, near, nz = [], [], [], 0, 0
    v = z
    for q in range(n_passes):
        vs.append(v)
        near += soft_ref.near_edge(M, v, labels, rho_max)
        nz += soft_ref.zeros(M, v, labels)
        c = ldpc_ref.stream(M, v, labels, rho_max)
        cells, L = ldpc_ref.cells(code, ldpc_ref.codewords(code, c))
        chans.append(c)
        rows.append(cells)
        if q + 1 == n_passes:
            break
        l_hat = decided_labels(cfg, code, labels, c, L) if feedback == "decoder" else rm.detect_labels(const, v)
        v = cnc_step(cfg, pp, z, const[l_hat])
    return np.stack(chans), np.stack(rows), np.stack(vs), near, nz


def reference(cfg, code, seed, trials, rho_max, n_passes, iters=(0,), incl_clean=False, feedback="decoder", chunk=8):
    """-> (counts [n, n_idx] int64, chan [n, n_passes, S log2 M] int8, rows [n, n_passes, 4] float64,
    z [n, S] complex128, near-edge count and exact zeros of every v_q)."""
    trials = np.asarray(trials, dtype=np.int64)
    pp = sim.point_params(cfg)
    counts, chans, rows, zs, near, nz = [], [], [], [], 0, 0
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            labels = d["labels"][j]
            z_csi = d["z_csi"][j] if "z_csi" in d else None
            c, dbg = sim.run_trial(cfg, labels, d["z_chan"][j], d["z_noise"][j], d["loc_u"][j], z_csi,
                                   sorted(set(int(k) for k in iters)), incl_clean, return_debug=True)
            ch, rw, _, ne, zz = trial(cfg, code, pp, labels, dbg["z"], rho_max, n_passes, feedback)
            counts.append(np.asarray(c, np.int64))
            chans.append(ch)
            rows.append(rw)
            zs.append(np.asarray(dbg["z"], np.complex128))
            near += ne
            nz += zz
    return np.asarray(counts), np.asarray(chans), np.asarray(rows), np.asarray(zs), near, nz
