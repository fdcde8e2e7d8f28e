"""The run calls at the limits ``include/mimo_engine.h`` documents, their case tables and cached
oracle references.  No GPU.

Three families, each the smallest system that reaches its limit:

* ``DEEP``: receivers run to iteration 31, the deepest the header allows, on systems whose
  feedback loops keep moving (period-2 cycles) or settle on a level with errors, so that every
  one of the 33 counter columns says something a shallower loop would not;
* ``LARGE``: 1024- and 4096-QAM (lattice levels up to |63|) on the instances that keep the
  symbols as packed levels -- int8 pairs at F 4096 float64, one word at F 2048, the LDS copy at
  F 8192;
* ``tiny_config``: one antenna on 4 sub-carriers at F 128, cheap enough per trial that a launch
  of 2^20 trials, and the spectrum mode's 256,140, run in seconds, while the oracle answers any
  trial index in milliseconds.

``tests/test_limit_cases.py`` pins, from the oracle alone, the conditions that make the tables
worth running; ``tests/test_gpu_iteration_lists.py``, ``tests/test_gpu_sizes.py`` and
``tests/test_gpu_full_launches.py`` run them on the device.  Eb/N0 converts as in
``tests/test_gpu_sizes.py``: ``ebn0_to_snr(ebn0, S, S, M)``.
"""
import functools

import numpy as np

from oracle import refmath as rm
from oracle import sim

FULL = list(range(32))                                    # every iteration the header allows
SPARSE = ([31], [0, 31], [5, 8], list(range(1, 9)))       # lists whose columns are not their iterations

# ---------------------------------------------------------------- deep iterations
DEEP_SEED = 41
# tag: A, S,    F,    M,  IBO, Eb/N0, channel,    receiver, trials, own list (None: FULL)
DEEP = {
    "D1": (8, 256, 512, 16, 0.0, 10.0, "rayleigh", "cnc", 12, None),    # cycling
    "D2": (8, 256, 512, 64, 1.0, 14.0, "rayleigh", "mcnc", 12, None),   # settling
    "D3": (4, 100, 256, 64, 0.0, 14.0, "rayleigh", "cnc", 12, None),    # cycling, generic slots
    "D4": (8, 256, 512, 16, 0.0, 9.0, "two_path", "cnc", 12, None),     # settling
    "D5": (4, 2048, 4096, 64, 3.0, 15.0, "rayleigh", "cnc", 3, None),   # 256-thread float64 team
    # 512-thread team.  Eb/N0 10 dB, not the 12 dB first tabled: there iterations 8 and 31 counted
    # the same in both trials (tests/test_limit_cases.py asks that they differ); here they differ in both
    "D6": (4, 4096, 8192, 16, 2.0, 10.0, "rayleigh", "mcnc", 2, (0, 8, 31)),
}
DEEP_TAGS = sorted(DEEP)
SMALL_TAGS = ["D1", "D2", "D3", "D4"]      # the cases cheap enough for every list and mode
SETTLING = ("D2", "D4")                    # float32 is asserted on all their columns
# what mimo_engine_describe reports for the float64 instance of each case
DEEP_DESCRIBE = {
    "D1": "F=512 T=64 slots=4 aligned ch=1 csi=0 f64",
    "D2": "F=512 T=64 slots=4 aligned ch=1 csi=0 f64",
    "D3": "F=256 T=64 slots=4 generic ch=1 csi=0 f64",
    "D4": "F=512 T=64 slots=4 aligned ch=3 csi=0 f64",
    "D5": "F=4096 T=256 slots=8 aligned ch=1 csi=0 f64",
    "D6": "F=8192 T=512 slots=8 aligned ch=1 csi=0 f64",
}


def deep_config(tag):
    """(SimConfig, number of trials, the case's iteration list) of a ``DEEP`` case."""
    A, S, F, M, ibo, ebn0, channel, receiver, n, own = DEEP[tag]
    cfg = sim.SimConfig(A, S, F, M, pa="softlim", ibo_db=ibo, snr_db=float(rm.ebn0_to_snr(ebn0, S, S, M)),
                        channel=channel, receiver=receiver)
    return cfg, n, list(own) if own else FULL


@functools.lru_cache(maxsize=None)
def deep_reference(tag, iters=None, incl_clean=True):
    """The oracle's per-trial counts [trials, n_idx] of a ``DEEP`` case for the tuple ``iters``
    (None: the case's own list); computed once, read-only."""
    cfg, n, own = deep_config(tag)
    ref = sim.run_trials(cfg, DEEP_SEED, np.arange(n), iters=list(iters) if iters is not None else own,
                         incl_clean=incl_clean, chunk=4)
    ref.setflags(write=False)
    return ref


def columns_of(iters, incl_clean, full_clean=True):
    """The columns of a ``FULL`` run (with clean if ``full_clean``) that the list ``iters`` records."""
    off = 1 if full_clean else 0
    return ([0] if incl_clean else []) + [off + i for i in iters]


def beam_probes():
    """9 probes (an odd list) for the beam mode: a 30 m half circle at the user's height."""
    th = np.deg2rad(np.arange(0.0, 181.0, 22.5))
    return np.stack([30.0 * np.cos(th), 30.0 * np.sin(th), np.full(th.shape, 1.5)], axis=1)


# ---------------------------------------------------------------- large constellations
LARGE_SEED = 7
LARGE_TRIALS = 3
LARGE_ITERS = [0, 1, 2]
# A, S,   F,    M,    Eb/N0, receiver, the oracle's totals [clean, it0, it1, it2]
LARGE = [
    (2, 2048, 4096, 4096, 40.0, "cnc", [8, 2300, 6020, 9191]),
    (2, 2048, 4096, 4096, 40.0, "mcnc", [8, 2300, 11, 7]),        # settling
    (2, 4096, 8192, 4096, 40.0, "cnc", [13, 5790, 13719, 20665]),
    (2, 4096, 8192, 1024, 32.0, "mcnc", [57, 671, 56, 58]),       # settling
    (2, 1024, 2048, 4096, 40.0, "cnc", [2, 1378, 2944, 4187]),
]
LARGE_NUMBERS = list(range(len(LARGE)))
LARGE_SETTLING = (1, 3)
LARGE_TEAM64 = {4096: 256, 8192: 512, 2048: 256}  # threads of the float64 team per FFT size


def large_id(i):
    A, S, F, M, ebn0, receiver, _ = LARGE[i]
    return f"F{F}-M{M}-{receiver}"


def large_config(i):
    A, S, F, M, ebn0, receiver, _ = LARGE[i]
    return sim.SimConfig(A, S, F, M, pa="softlim", ibo_db=6.0, snr_db=float(rm.ebn0_to_snr(ebn0, S, S, M)),
                         receiver=receiver)


@functools.lru_cache(maxsize=None)
def large_reference(i):
    ref = sim.run_trials(large_config(i), LARGE_SEED, np.arange(LARGE_TRIALS), iters=LARGE_ITERS, incl_clean=True,
                         chunk=1)
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------- full launches
TINY_SEED = 3
TINY_ITERS = [0, 2]
LAUNCH = 1 << 20                         # trials of one launch (engine.hip plan_launches)
SLICE = 4096                             # trials of one reduction slice (engine.hip kSlice)
# the edges of a slice and of a launch
TINY_OFFSETS = [0, 1, SLICE - 1, SLICE, SLICE + 1, LAUNCH - 1, LAUNCH, LAUNCH + 1, LAUNCH + 2]
# the oracle's rows [clean, it0, it2] at trial = offset
TINY_ROWS = [[0, 1, 1], [0, 1, 0], [4, 4, 4], [2, 2, 1], [1, 3, 3], [3, 3, 2], [1, 2, 1], [1, 2, 0], [1, 0, 0]]
SPEC_BUFFER_BYTES = 256 << 20            # include/mimo_engine.h MIMO_SPEC_BUFFER_BYTES
SPEC_FIXED = 3                           # include/mimo_engine.h MIMO_SPEC_FIXED


def tiny_config(ibo_db=-2.0):
    return sim.SimConfig(1, 4, 128, 16, pa="softlim", ibo_db=ibo_db, snr_db=float(rm.ebn0_to_snr(6, 4, 4, 16)))


def tiny_rows(trials, seed=TINY_SEED, ibo_db=-2.0, incl_clean=True):
    """The oracle's rows of the tiny system at the given trial indices."""
    return sim.run_trials(tiny_config(ibo_db), seed, np.asarray(trials, np.int64), iters=TINY_ITERS,
                          incl_clean=incl_clean, chunk=64)


def sample_offsets(n, count=64, seed=20):
    """``count`` further offsets below ``n`` from a fixed-seed draw, sorted."""
    return np.sort(np.random.default_rng(seed).choice(n, size=count, replace=False))
