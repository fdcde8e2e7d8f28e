"""The mixed-point launch of tests/test_gpu_point_fields.py: one list of grid points in which every
``mimo_point`` field the kernels fetch per block differs between neighbours, with the float64
oracle's counts for it.

The kernels read a block's parameters from ``points[pi]`` after a search over ``point_start``; a
kernel that took a field from point 0, from the launch parameters or from the wrong sibling
(``sat_cnc`` for ``sat_tx``, ``toi_cnc`` for ``toi_tx``) counts differently on this list -- which
``neighbours_differ`` / ``mismatch_differs`` establish on the oracle alone, as a condition on the
inputs: every point's trials, run under the parameters of the point before or after it, give
other counts than under its own.
"""
import functools

import numpy as np

from oracle import refmath as rm
from oracle import sim

ITERS = (0, 1, 2)
CLEAN = True

# (SimConfig overrides, n_trials, seed, first_trial), in launch order
MIX = [
    (dict(pa="softlim", ibo_db=1.0), 3, 100, 0),
    (dict(pa="rapp", p_hardness=3.0, ibo_db=1.0), 3, 101, 5),           # rapp_int<3>
    (dict(pa="toi", ibo_db=6.0), 3, 102, 1000),                          # sat_pow = 0
    (dict(pa="rapp", p_hardness=2.5, ibo_db=1.0), 3, 103, 17),          # the general Rapp, out of line
    (dict(pa="none", ibo_db=1.0), 3, 104, 2),
    (dict(pa="rapp", p_hardness=2.0, ibo_db=2.0), 3, 105, (1 << 32) - 3),  # rapp_int<2>; the last trial ids
    (dict(pa="softlim", ibo_db=1.0, array_alpha=0.93, cnc_alpha=0.93), 3, 106, 40),  # constant alpha polynomial
    (dict(pa="rapp", p_hardness=3.0, ibo_db=1.0, cnc_pa="softlim", cnc_ibo_db=1.0), 4, 107, 0),  # kind mismatch
    (dict(pa="softlim", ibo_db=1.0, cnc_ibo_db=2.5, cnc_alpha=0.9), 5, 108, 9),   # sat_cnc != sat_tx
    (dict(pa="toi", ibo_db=6.0, cnc_pa="toi", cnc_ibo_db=3.0), 2, 109, 300),       # toi_cnc != toi_tx
    (dict(pa="softlim", ibo_db=3.0), 0, 110, 77),                        # no trials
]
ZERO_TRIAL_POINT = 10
MISMATCH = (7, 8, 9)           # the receiver's PA is not the array's
BASE = range(7)                # points 0-6: receiver = array
RECEIVER_FIELDS = ("cnc_pa", "cnc_ibo_db", "cnc_toi_coeff", "cnc_alpha")

# (n_ant, n_sc, n_fft, M, Eb/N0 [dB]): the smallest instance of each slot / FFT family
SHAPES = {
    "f512_aligned": (8, 256, 512, 16, 12.0),     # aligned slots, one wave
    "f256_generic": (4, 100, 256, 64, 16.0),     # generic slots, a band that is no multiple of the team
    # float64: the wave-split FFT at T 256 (float32: T 128, 8 slots); several waves share the point index
    "f2048_wave": (4, 1024, 2048, 64, 16.0),
}


def base_config(shape, **kw):
    a, s, f, m, ebn0 = SHAPES[shape]
    # the drivers' Eb/N0 -> SNR (utilities.ebn0_to_snr with n_fft = n_sub_carr, as they call it)
    return sim.SimConfig(a, s, f, m, snr_db=float(rm.ebn0_to_snr(ebn0, s, s, m)), **kw)


def configs(shape, receiver="cnc", which=None):
    idx = range(len(MIX)) if which is None else which
    return [base_config(shape, receiver=receiver, **MIX[i][0]) for i in idx]


def launch_args(which=None):
    """(seeds, first_trials, n_trials) of the points ``which`` (all by default)."""
    idx = range(len(MIX)) if which is None else which
    return [MIX[i][2] for i in idx], [MIX[i][3] for i in idx], [MIX[i][1] for i in idx]


def point_of(cfg):
    """The mimo_point keywords of an oracle config (gpu_util.engine_for's, without an engine)."""
    pp = sim.point_params(cfg)
    avg = pp["avg_samp"] / cfg.n_ant  # MRT: mean |P|^2 = 1/A
    kw = dict(toi_coeff=rm.toi_coeff(cfg.ibo_db, avg)) if cfg.pa == "toi" else dict(sat_pow=rm.sat_pow(cfg.ibo_db, avg))
    return dict(ibo_db=cfg.ibo_db, snr_db=cfg.snr_db, avg_symbol_power=pp["es"], pa_kind=cfg.pa,
                p_hardness=cfg.p_hardness, cnc_pa_kind=pp["cnc_pa"], cnc_sat_pow=pp["cnc_sat"],
                cnc_toi_coeff=pp["cnc_coeff"], cnc_alpha=pp["cnc_alpha"], csi_eps=cfg.csi_eps,
                array_alpha=cfg.array_alpha, **kw)


def _frozen(a):
    a = np.asarray(a, np.int64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_counts(shape, i, under=None, receiver="cnc"):
    """Counts [n_trials, n_idx] of point i's trials under point ``under``'s parameters (its own by
    default).  Computed once per process and shared read-only."""
    cfg = base_config(shape, receiver=receiver, **MIX[i if under is None else under][0])
    _, n, seed, first = MIX[i]
    if n == 0:
        return _frozen(np.zeros((0, len(ITERS) + int(CLEAN))))
    return _frozen(sim.run_trials(cfg, seed, np.arange(first, first + n), iters=ITERS, incl_clean=CLEAN))


def matched(i):
    """Point i's overrides with the receiver fields left to follow the array's."""
    return {k: v for k, v in MIX[i][0].items() if k not in RECEIVER_FIELDS}


@functools.lru_cache(maxsize=None)
def oracle_counts_matched(shape, i):
    """Counts of point i's trials with a receiver whose PA copy is the array's."""
    cfg = base_config(shape, **matched(i))
    _, n, seed, first = MIX[i]
    return _frozen(sim.run_trials(cfg, seed, np.arange(first, first + n), iters=ITERS, incl_clean=CLEAN))


def neighbours_differ(shape, receiver="cnc", which=None):
    """[] if every point's counts change under each neighbour's parameters, else the (i, j) that do not."""
    idx = list(range(len(MIX))) if which is None else list(which)
    same = []
    for k, i in enumerate(idx):
        if MIX[i][1] == 0:
            continue
        for j in idx[max(0, k - 1):k] + idx[k + 1:k + 2]:
            if np.array_equal(oracle_counts(shape, i, None, receiver), oracle_counts(shape, i, j, receiver)):
                same.append((i, j))
    return same


def mismatch_differs(shape):
    """[] if every mismatch point counts differently from its matched-receiver twin."""
    return [i for i in MISMATCH if np.array_equal(oracle_counts(shape, i), oracle_counts_matched(shape, i))]
