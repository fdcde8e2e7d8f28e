"""Reference for the engine's coded mode (mimo_engine_coded_points, mimo_ldpc_decode): a numpy
restatement of the definitions next to ``mimo_ldpc_code`` in include/mimo_engine.h.

Everything is integer after the one ``floor`` of the quantiser: the channel value
``c = 2 clamp(floor(rho scale), -32, 31) + 1`` with ``scale = 32.0 / rho_max`` on the soft mode's
reliability ``rho`` (``soft_ref.rho``), the bit stream ``p = j S + k`` of one trial and counter
index, its ``n_cw`` interleaved codewords (bit ``n`` of codeword ``w`` at ``n n_cw + w``), the layered
normalised min-sum decoder with messages kept per edge (no compressed check state), the hard
decision, the syndrome and the four cells of a row.
"""
import numpy as np

import soft_ref
from oracle import sim

CODED_FIXED = 4


class Code:
    """A QC-LDPC code: ``shifts`` [n_rows, n_cols] int16, -1 = zero block."""

    def __init__(self, z, shifts, n_dec_iters=10):
        self.z, self.n_dec_iters = int(z), int(n_dec_iters)
        self.shifts = np.array(shifts, np.int16)
        self.n_rows, self.n_cols = self.shifts.shape

    @property
    def n_bits(self):
        return self.n_cols * self.z

    def layers(self):
        """Per base row the bit indices [n_edges, z] of its checks: check i touches bit
        c z + (i + s) mod z of every base column c whose shift s is not -1."""
        i = np.arange(self.z)
        return [np.stack([c * self.z + (i + int(s)) % self.z for c, s in enumerate(row) if s >= 0])
                for row in self.shifts]

    def with_iters(self, n):
        return Code(self.z, self.shifts, n)


def quantise(rho, rho_max):
    """c = 2 clamp(floor(rho * scale), -32, 31) + 1, scale = 32.0 / rho_max, the clamp in double."""
    scale = np.float64(32.0) / np.float64(rho_max)
    f = np.floor(np.asarray(rho, np.float64) * scale)
    return (2 * np.clip(f, -32.0, 31.0).astype(np.int64) + 1).astype(np.int8)


def stream(constel_size, v, labels, rho_max):
    """The channel values of one trial and counter index, [log2 M * S] int8: Gray bit j (the I axis
    MSB first, then Q: ``soft_ref.rho``'s columns) of sub-carrier k at j S + k."""
    return quantise(soft_ref.rho(constel_size, v, labels), rho_max).T.reshape(-1)


def codewords(code, chan):
    """[n_cw, N] from a stream (or [..., stream]): bit n of codeword w is position n n_cw + w."""
    chan = np.asarray(chan)
    n_cw = chan.shape[-1] // code.n_bits
    cut = chan[..., :n_cw * code.n_bits]
    return np.swapaxes(cut.reshape(chan.shape[:-1] + (code.n_bits, n_cw)), -1, -2)


def decode(code, chan):
    """Final L [n, N] int16 of the codewords ``chan`` [n, N] (any integers with |c| <= 63)."""
    L = np.array(chan, np.int64).reshape(-1, code.n_bits)
    assert np.abs(L).max(initial=0) <= 63
    layers = code.layers()
    R = [np.zeros((L.shape[0],) + idx.shape, np.int64) for idx in layers]
    for _ in range(code.n_dec_iters):
        for r, idx in enumerate(layers):
            T = L[:, idx] - R[r]                       # [n, edges, z]
            a = np.abs(T)
            order = np.argsort(a, axis=1, kind="stable")
            m1 = np.take_along_axis(a, order[:, :1], axis=1)
            m2 = np.take_along_axis(a, order[:, 1:2], axis=1)
            e = np.arange(idx.shape[0])[None, :, None]
            m = np.where(e == order[:, :1], m2, m1)    # the smallest |T| of the other edges
            neg = T < 0
            odd = (neg.sum(axis=1, keepdims=True) - neg) & 1
            R[r] = np.where(odd == 1, -1, 1) * np.minimum(127, (3 * m) >> 2)
            L[:, idx] = T + R[r]
    assert np.abs(L).max(initial=0) <= 63 + 127 * code.n_rows
    return L.astype(np.int16)


def syndrome(code, L):
    """[n] bool: the hard decision (1 iff L < 0) of each codeword fails a check."""
    hard = np.asarray(L).reshape(-1, code.n_bits) < 0
    bad = np.zeros(hard.shape[0], bool)
    for idx in code.layers():
        bad |= (hard[:, idx].sum(axis=1) & 1).any(axis=1)
    return bad


def cells(code, chan):
    """The four cells over the codewords ``chan`` [n_cw, N], and their final L."""
    L = decode(code, chan)
    wrong = (L < 0).sum(axis=1)
    return np.array([(np.asarray(chan) < 0).sum(), wrong.sum(), (wrong > 0).sum(), syndrome(code, L).sum()],
                    np.float64), L


def n_codewords(n_sc, constel_size, code):
    return (n_sc * int(round(np.log2(constel_size)))) // code.n_bits


def reference(cfg, code, seed, trials, iters, rho_max, incl_clean=False, chunk=8):
    """-> (counts [n, n_idx] int64, chan [n, n_idx, S log2 M] int8, rows [n, n_idx, 4] float64,
    uncoded errors at the decoded positions [n, n_idx], near-edge count, exact zeros); the slicer
    inputs are ``soft_ref.slicer_inputs``'s."""
    trials = np.asarray(trials, dtype=np.int64)
    M = cfg.constel_size
    counts, chans, rows, dec_err, near, nz = [], [], [], [], 0, 0
    for i in range(0, len(trials), chunk):
        d = sim.draws(cfg, seed, trials[i:i + chunk])
        for j in range(len(trials[i:i + chunk])):
            c, labels, vs = soft_ref.slicer_inputs(cfg, d, j, iters, incl_clean)
            counts.append(c)
            ch = np.stack([stream(M, v, labels, rho_max) for v in vs])
            chans.append(ch)
            rows.append(np.stack([cells(code, codewords(code, s))[0] for s in ch]))
            # the oracle's decisions at the decoded positions: rho < 0 is a hard-decision error
            n_dec = n_codewords(cfg.n_sc, M, code) * code.n_bits
            dec_err.append([int((soft_ref.rho(M, v, labels).T.reshape(-1)[:n_dec] < 0).sum()) for v in vs])
            # (the 64 coded bins are 4 soft bins wide each: their edges are soft edges at the same
            # rho_max, so soft_ref's near-edge test covers them)
            near += sum(soft_ref.near_edge(M, v, labels, rho_max) for v in vs)
            nz += sum(soft_ref.zeros(M, v, labels) for v in vs)
    return (np.asarray(counts), np.asarray(chans), np.asarray(rows), np.asarray(dec_err, np.int64), near, nz)
