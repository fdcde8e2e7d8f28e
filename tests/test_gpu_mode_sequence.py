"""The four run modes on one engine, one after the other: the row modes share one pair of device
buffers (per-trial rows, slice partials), so a call must not see what a call of another mode, with
wider or narrower rows or more trials, left in them.  Every array a call returns -- counts, totals
and per-trial rows -- equals, bit for bit, the same call on a fresh engine.
"""
import numpy as np
import pytest

from gpu_util import engine_for
from oracle import sim
from test_gpu_beam import probes_n

pytestmark = pytest.mark.gpu

SEED = 7
ITERS = (0, 1)
# the smallest generic shape of the mode tests: a band that is not a multiple of a wave
CFG = sim.SimConfig(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                    channel="rayleigh")
MODES = ("plain", "measure", "spectrum", "beam")  # rows of 0, 7, 259 and 45 doubles


def call(eng, mode, first, n):
    if mode == "plain":
        return eng.run(SEED, first, n, ITERS, per_trial=True)
    if mode == "beam":
        return eng.beam(SEED, first, n, ITERS, probes_n(9), per_trial=True)
    return getattr(eng, mode)(SEED, first, n, ITERS, per_trial=True)


def assert_sequence_equals_fresh(eng, modes, first, n):
    for mode in modes:
        got = call(eng, mode, first, n)
        fresh = engine_for(CFG, precision="f64")
        want = call(fresh, mode, first, n)
        fresh.close()
        assert len(got) == len(want) == (3 if mode == "plain" else 5)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g is not None and g.shape[0] > 0
            np.testing.assert_array_equal(g, w, err_msg=f"{mode} first={first} n={n} output {k}")


def test_modes_in_sequence_equal_fresh_engines(monkeypatch):
    eng = engine_for(CFG, precision="f64")
    assert_sequence_equals_fresh(eng, MODES, 0, 11)
    assert_sequence_equals_fresh(eng, MODES[::-1], 16, 5)
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "3")  # four launches a call, in buffers that were larger
    assert_sequence_equals_fresh(eng, MODES, 0, 11)
    eng.close()
