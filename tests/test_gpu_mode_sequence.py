"""The seven run modes on one engine, one after the other: the row modes share one pair of device
buffers (per-trial rows, slice partials) -- the soft rows are the widest of them -- and the beam and
the coded mode add the buffer their second kernel reads and its tables, so a call must not see what
a call of another mode, with wider or narrower rows or more trials, left in them, nor leave anything
a later call sees.  Every array a call returns -- counts, totals, per-trial rows, the coded mode's
channel values -- equals, bit for bit, the same call on a fresh engine.
"""
import numpy as np
import pytest

from gpu_util import engine_for
from oracle import sim
from test_gpu_beam import probes_n
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu

SEED = 7
ITERS = (0, 1)
RHO_MAX = 16.0
# the smallest generic shape of the mode tests: a band that is not a multiple of a wave
CFG = sim.SimConfig(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                    channel="rayleigh")
# rows of 0, 7, 259, 45, 260, 768 and 12 doubles
MODES = ("plain", "measure", "spectrum", "beam", "envelope", "soft", "coded")
N_OUT = {"plain": 3, "coded": 6}  # arrays a call returns; the other modes 5
# Rows of counts (integers in doubles): however a call is split into launches, its totals are the
# same bits.  The other modes' rows hold sums of doubles, added launch by launch.
COUNTS_ONLY = ("plain", "soft", "coded")
CODE = qc_ldpc_code(16, 3, 6)       # 6 codewords a trial, 24 bits left over
OTHER_CODE = qc_ldpc_code(61, 3, 6)  # one codeword: other tables in the same device buffer


def call(eng, mode, first, n, code=CODE):
    if mode == "plain":
        return eng.run(SEED, first, n, ITERS, per_trial=True)
    if mode == "beam":
        return eng.beam(SEED, first, n, ITERS, probes_n(9), per_trial=True)
    if mode == "envelope":
        return eng.envelope(SEED, first, n, ITERS, 1.0, per_trial=True)
    if mode == "soft":
        return eng.soft(SEED, first, n, ITERS, RHO_MAX, incl_clean=True, per_trial=True)
    if mode == "coded":
        return eng.coded(SEED, first, n, ITERS, code, RHO_MAX, incl_clean=True, per_trial=True, chan=True)
    return getattr(eng, mode)(SEED, first, n, ITERS, per_trial=True)


def new_fresh(mode, first, n, code=CODE):
    eng = engine_for(CFG, precision="f64")
    out = call(eng, mode, first, n, code)
    eng.close()
    return out


_FRESH = {}


def fresh(mode, first, n):
    """The call on a fresh engine, made once per module (before any test lowers the launch size) and
    left unchanged."""
    if (mode, first, n) not in _FRESH:
        _FRESH[mode, first, n] = new_fresh(mode, first, n)
    return _FRESH[mode, first, n]


def assert_same(got, want, label, mode):
    assert len(got) == len(want) == N_OUT.get(mode, 5)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g is not None and g.shape[0] > 0
        np.testing.assert_array_equal(g, w, err_msg=f"{label} output {k}")


def assert_second_kernel_times(eng, mode):
    """The second kernel's time is the last call's: none where the mode has no such kernel."""
    assert (eng.decode_kernel_ms > 0) == (mode == "coded")
    assert (eng.beam_kernel_ms > 0) == (mode == "beam")


def assert_sequence_equals_fresh(eng, modes, first, n, want=fresh):
    for mode in modes:
        assert_same(call(eng, mode, first, n), want(mode, first, n), f"{mode} first={first} n={n}", mode)
        assert_second_kernel_times(eng, mode)


def test_modes_in_sequence_equal_fresh_engines(monkeypatch):
    for mode in MODES:  # the references, at the full launch size
        fresh(mode, 0, 11)
    eng = engine_for(CFG, precision="f64")
    assert_sequence_equals_fresh(eng, MODES, 0, 11)
    assert_sequence_equals_fresh(eng, MODES[::-1], 16, 5)
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "3")  # four launches a call, in buffers that were larger
    assert_sequence_equals_fresh(eng, MODES, 0, 11, want=new_fresh)    # ... equal a fresh engine's four
    assert_sequence_equals_fresh(eng, COUNTS_ONLY, 0, 11)              # ... and, for counts, the one launch
    eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_mode_between_the_other_modes_equals_fresh_engines(mode, monkeypatch):
    """A call of the mode before and after a call of each other mode returns what a fresh engine
    returns, and so does the other mode's call between them."""
    want = {(0, 11): fresh(mode, 0, 11), (16, 5): fresh(mode, 16, 5)}
    others = [m for m in MODES if m != mode]
    for other in others:
        fresh(other, 16, 7)
    eng = engine_for(CFG, precision="f64")
    for other in others:
        assert_same(call(eng, mode, 0, 11), want[(0, 11)], f"{mode} before {other}", mode)
        assert_second_kernel_times(eng, mode)
        assert_same(call(eng, other, 16, 7), fresh(other, 16, 7), f"{other} after {mode}", other)
        assert_second_kernel_times(eng, other)
        assert_same(call(eng, mode, 16, 5), want[(16, 5)], f"{mode} after {other}", mode)
    if mode == "coded":  # another code on the same engine, then the first again
        assert_same(call(eng, "coded", 0, 11, OTHER_CODE), new_fresh("coded", 0, 11, OTHER_CODE),
                    "coded with another code", mode)
        assert_same(call(eng, "coded", 0, 11), want[(0, 11)], "coded after another code", mode)
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "3")  # four launches a call, in buffers that were larger
    assert_same(call(eng, mode, 0, 11), want[(0, 11)] if mode in COUNTS_ONLY else new_fresh(mode, 0, 11),
                f"{mode} in four launches", mode)
    eng.close()
