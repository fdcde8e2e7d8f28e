"""The turbo mode's step kernel through its seam (mimo_engine_cnc_step) against the fused kernel's CNC
loop: with hard slices as the decisions the step is one CNC iteration, so from the device's own
received vectors (``per_trial_z`` of a turbo call) two rounds of slice -> cnc_step -> slice give, per
trial, exactly the error counts the plain run records at iterations 1 and 2.  Decisions must agree;
bitwise equality of ``v`` is not asked for.  Every FFT kind of the float64 instances (one wave,
T 64 with 8 points, the wave-split teams, the 16-point team, the split FFT), aligned and generic bands
and every receiver PA model.
"""
import functools

import numpy as np
import pytest

import _engine
import soft_ref
import turbo_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import refmath as rm
from oracle import sim
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu

SEED, N_TRIALS = 7, 8
BASE = dict(constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0, channel="rayleigh")
CASES = {
    "f128_generic": dict(BASE, n_ant=4, n_sc=64, n_fft=128),                               # one wave, P 2
    "f256_generic_odd": dict(BASE, n_ant=4, n_sc=100, n_fft=256, constel_size=64, snr_db=25.0),
    "f512_aligned": dict(BASE, n_ant=8, n_sc=256, n_fft=512),                              # T 64, P 8, 4 slots
    "f512_generic_toi": dict(BASE, n_ant=4, n_sc=300, n_fft=512, pa="toi", ibo_db=6.0),
    "f512_rapp25": dict(BASE, n_ant=8, n_sc=256, n_fft=512, pa="rapp", p_hardness=2.5),    # the cold Rapp path
    "f1024_aligned": dict(BASE, n_ant=2, n_sc=512, n_fft=1024),                            # wave-split T 128
    "f1024_generic": dict(BASE, n_ant=2, n_sc=600, n_fft=1024),
    "f2048_aligned_rapp3": dict(BASE, n_ant=2, n_sc=1024, n_fft=2048, pa="rapp", p_hardness=3.0),  # wave-split T 256
    "f2048_generic": dict(BASE, n_ant=2, n_sc=1200, n_fft=2048),
    "f4096_8slots_rapp3": dict(BASE, n_ant=2, n_sc=2048, n_fft=4096, pa="rapp", p_hardness=3.0),   # 16-point team
    "f4096_4slots": dict(BASE, n_ant=2, n_sc=1024, n_fft=4096),
    "f8192_8slots": dict(BASE, n_ant=2, n_sc=4096, n_fft=8192),                            # split FFT
    "f8192_generic_toi": dict(BASE, n_ant=2, n_sc=3000, n_fft=8192, pa="toi", ibo_db=6.0),
}


@functools.lru_cache(maxsize=None)
def small_code():
    return _engine.LdpcCode(16, np.array(qc_ldpc_code(16, 3, 6).table), 2)


def errors(cfg, labels_hat, labels_tx):
    nb = int(np.log2(cfg.constel_size))
    x = np.bitwise_xor(np.asarray(labels_hat, np.int64), np.asarray(labels_tx, np.int64))
    return sum(((x >> j) & 1) for j in range(nb)).sum(axis=1)


def received(eng):
    """The device's own z of trials 0 .. N_TRIALS - 1 (a one-pass turbo call)."""
    return eng.turbo(SEED, 0, N_TRIALS, (0,), small_code(), 16.0, 1, z=True)[-1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_rounds_of_the_seam_are_cnc_iterations_1_and_2(name):
    cfg = sim.SimConfig(**CASES[name])
    pp = sim.point_params(cfg)
    eng = engine_for(cfg, precision="f64")
    M, S = cfg.constel_size, cfg.n_sc
    labels_tx = sim.draws(cfg, SEED, np.arange(N_TRIALS))["labels"]
    _, _, per_run = eng.run(SEED, 0, N_TRIALS, (0, 1, 2), per_trial=True)
    z = received(eng)
    lab0 = _engine.qam_slice(M, z).reshape(N_TRIALS, S)
    v1 = eng.cnc_step(z, lab0)
    lab1 = _engine.qam_slice(M, v1).reshape(N_TRIALS, S)
    v2 = eng.cnc_step(z, lab1)
    lab2 = _engine.qam_slice(M, v2).reshape(N_TRIALS, S)
    got = np.stack([errors(cfg, lab, labels_tx) for lab in (lab0, lab1, lab2)], axis=1)
    print(name, eng.describe(), "seam", got.sum(0), "run", per_run.sum(0))
    assert_counts_equal(got, per_run, f"{name}: slice / cnc_step rounds vs the fused loop")
    # ... and the step is the reference's, within the allowance of the received vector
    ref1 = np.stack([turbo_ref.cnc_step(cfg, pp, z[i], pp["const"][lab0[i]]) for i in range(N_TRIALS)])
    assert np.abs(v1 - ref1).max() <= soft_ref.EPS_V * np.abs(z).max()
    eng.close()


@pytest.mark.parametrize("name", ["f512_aligned", "f256_generic_odd", "f2048_aligned_rapp3"])
def test_transmitted_labels_give_one_distortion_whatever_the_noise(name):
    """dist depends on the decisions alone: with the transmitted labels, z - v is the same vector at
    two SNRs (two noise levels of the same trials), up to the rounding of the subtraction."""
    cfg = sim.SimConfig(**CASES[name])
    labels_tx = sim.draws(cfg, SEED, np.arange(N_TRIALS))["labels"]
    eng = engine_for(cfg, precision="f64")
    z_a = received(eng)
    eng.set_point(**dict(eng.point_kw, snr_db=cfg.snr_db - 10.0))
    z_b = received(eng)
    assert np.abs(z_a - z_b).max() > 1e-3  # the noise did change
    d_a, d_b = z_a - eng.cnc_step(z_a, labels_tx), z_b - eng.cnc_step(z_b, labels_tx)
    eng.close()
    scale = max(np.abs(z_a).max(), np.abs(z_b).max())
    assert np.abs(d_a - d_b).max() <= 8 * np.finfo(np.float64).eps * scale
    assert np.abs(d_a).max() > 1e-3  # and there is a distortion to subtract


def test_step_of_many_rows_equals_row_by_row():
    cfg = sim.SimConfig(**CASES["f1024_generic"])
    eng = engine_for(cfg, precision="f64")
    z = received(eng)
    lab = _engine.qam_slice(cfg.constel_size, z).reshape(N_TRIALS, cfg.n_sc)
    whole = eng.cnc_step(z, lab)
    for i in (0, N_TRIALS - 1):
        np.testing.assert_array_equal(eng.cnc_step(z[i], lab[i])[0], whole[i])
    eng.close()
