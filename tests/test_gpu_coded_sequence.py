"""The coded mode among the other run modes on one engine: the row modes share one pair of device
buffers (per-trial rows, slice partials), and the coded mode adds its channel-value buffer and the
decoder's tables, so a coded call must not see what a call of another mode left there, nor leave
anything a later call sees.  A coded call before and after a call of each other mode returns, bit
for bit, what a fresh engine returns, and so does the other mode's call between them.
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
OTHERS = ("plain", "measure", "spectrum", "beam", "envelope", "soft")
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


def fresh(mode, first, n, code=CODE):
    eng = engine_for(CFG, precision="f64")
    out = call(eng, mode, first, n, code)
    eng.close()
    return out


def assert_same(got, want, label):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g is not None and g.shape[0] > 0
        np.testing.assert_array_equal(g, w, err_msg=f"{label} output {k}")


def test_coded_between_the_other_modes_equals_fresh_engines(monkeypatch):
    want = {(0, 11): fresh("coded", 0, 11), (16, 5): fresh("coded", 16, 5)}
    eng = engine_for(CFG, precision="f64")
    for mode in OTHERS:
        assert_same(call(eng, "coded", 0, 11), want[(0, 11)], f"coded before {mode}")
        assert eng.decode_kernel_ms > 0
        assert_same(call(eng, mode, 16, 7), fresh(mode, 16, 7), f"{mode} after coded")
        assert eng.decode_kernel_ms == 0
        assert_same(call(eng, "coded", 16, 5), want[(16, 5)], f"coded after {mode}")
    # another code on the same engine, then the first again
    assert_same(call(eng, "coded", 0, 11, OTHER_CODE), fresh("coded", 0, 11, OTHER_CODE), "coded with another code")
    assert_same(call(eng, "coded", 0, 11), want[(0, 11)], "coded after another code")
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "3")  # four launches a call, in buffers that were larger
    assert_same(call(eng, "coded", 0, 11), want[(0, 11)], "coded in four launches")
    eng.close()
