"""Turbo mode (mimo_engine_turbo_points) on the GPU: the same counts as the plain run and the oracle,
and per trial and pass of the decoder-aided CNC receiver the channel values of every stream position
equal to the oracle-built reference (tests/turbo_ref.py) byte for byte and the four cells of the
LDPC-decoded link equal to the reference decoder's, cell for cell.

The systems are tests/test_gpu_soft.py's ``CASES``, by value (``rho_max`` 16, seed 7), the codes
tests/test_gpu_coded.py's tables at 10 decoder iterations; ``n_passes`` 3, 4 for the LoS case.  The
comparison is exact under the soft mode's conditions -- no reliability of any ``v_q`` within the
allowed error of a bin edge (``near == 0``), none exactly 0 -- which every case asserts on the
reference before it looks at the device, with the reference's totals per pass (the issue's record).
"""
import dataclasses
import functools

import numpy as np
import pytest

import _engine
import ldpc_ref
import soft_ref
import turbo_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import sim
from test_gpu_ldpc_seam import punched_128
from test_gpu_soft import CASES as SOFT_CASES
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu

N_TRIALS = 8
N_DEC = 10
SEED = 7
RHO_MAX = 16.0
TABLES = {
    "z16": (16, lambda: qc_ldpc_code(16, 3, 6).table),
    "z61": (61, lambda: qc_ldpc_code(61, 3, 6).table),
    "z64": (64, lambda: qc_ldpc_code(64, 4, 8).table),
    "z128": (128, punched_128),
    "z512": (512, lambda: qc_ldpc_code(512, 12, 24).table),
}
F1024 = dict(n_ant=2, n_sc=512, n_fft=1024, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0, channel="rayleigh")
LOS = dict(SOFT_CASES["f512_los"][0], ibo_db=0.0, snr_db=20.0)
# case -> (config, iteration list and clean run of the counts, code, n_passes, decoded bits, n_cw,
#          the reference's totals per pass: the issue's record)
CASES = {
    # one wave, hb 1, a tail of 32 bits
    "f128_qpsk-z16": (SOFT_CASES["f128_qpsk"][0], (0, 1), False, "z16", 3, 96, 1,
                      [(16, 0, 0, 0), (17, 0, 0, 0), (17, 0, 0, 0)]),
    # generic band, odd z, a tail of 234
    "f256_generic-z61": (SOFT_CASES["f256_generic"][0], (0, 1, 2), True, "z61", 3, 366, 1,
                         [(16, 0, 0, 0), (112, 0, 0, 0), (130, 0, 0, 0)]),
    # generic band, 6 codewords
    "f256_generic-z16": (SOFT_CASES["f256_generic"][0], (0, 1, 2), True, "z16", 3, 576, 6,
                         [(24, 0, 0, 0), (171, 0, 0, 0), (176, 0, 0, 0)]),
    # the CSI instance, 2 codewords
    "f512_csi-z64": (SOFT_CASES["f512_csi"][0], (0, 1), True, "z64", 3, 1024, 2,
                     [(13, 0, 0, 0), (31, 0, 0, 0), (31, 0, 0, 0)]),
    # the gain: frames corrected
    "f512_los-z64": (LOS, (0, 1), False, "z64", 4, 1536, 3,
                     [(1191, 102, 3, 3), (183, 0, 0, 0), (144, 0, 0, 0), (144, 0, 0, 0)]),
    # the cold (general-hardness) Rapp path in the step kernel
    "f512_los_rapp-z64": (dict(LOS, pa="rapp", p_hardness=2.5), (0, 1), False, "z64", 3, 1536, 3,
                          [(1104, 0, 0, 0), (115, 0, 0, 0), (115, 0, 0, 0)]),
    # wave-split T 128
    "f1024-z64": (F1024, (0, 1), False, "z64", 3, 2048, 4, [(84, 0, 0, 0), (163, 0, 0, 0), (163, 0, 0, 0)]),
    # wave-split T 256, irregular rows
    "f2048-z128": (dict(SOFT_CASES["f2048_mcnc"][0], receiver="cnc"), (0, 1, 2), False, "z128", 3, 6144, 6,
                   [(182, 0, 0, 0), (1524, 0, 0, 0), (1524, 0, 0, 0)]),
    # 16-point team, Rapp p 3, 12 codewords
    "f4096_rapp-z128": (SOFT_CASES["f4096_rapp"][0], (0, 1), False, "z128", 3, 12288, 12,
                        [(1718, 0, 0, 0), (3878, 0, 0, 0), (3878, 0, 0, 0)]),
    # split FFT, the largest decoder state
    "f8192-z512": (SOFT_CASES["f8192"][0], (0, 1), False, "z512", 3, 24576, 2,
                   [(2678, 0, 0, 0), (8450, 0, 0, 0), (8450, 0, 0, 0)]),
}


@functools.lru_cache(maxsize=None)
def codes(key):
    """(the engine's LdpcCode, the reference's Code) of a table."""
    z, table = TABLES[key]
    t = np.array(table())
    return _engine.LdpcCode(z, t, N_DEC), ldpc_ref.Code(z, t, N_DEC)


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS):
    """(config, counts, channel values [n, n_passes, stream], rows [n, n_passes, 4], z [n, S], near-edge
    count, exact zeros) of a case."""
    kw, iters, clean, key, n_passes, _, _, _ = CASES[name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    out = turbo_ref.reference(cfg, codes(key)[1], SEED, np.arange(first, first + n), RHO_MAX, n_passes, iters, clean)
    for a in out[:4]:
        a.setflags(write=False)
    return (cfg,) + out


def assert_reference_conditions(name, cfg, counts, chan, rows, z, near, nz, totals=True):
    """The conditions on the inputs, on the reference alone."""
    _, _, _, key, n_passes, n_dec, n_cw, want = CASES[name]
    ref_code = codes(key)[1]
    assert near == 0, f"{name}: {near} reliabilities near a bin edge"
    assert nz == 0, f"{name}: {nz} reliabilities are exactly 0"
    assert (ldpc_ref.n_codewords(cfg.n_sc, cfg.constel_size, ref_code), n_cw * ref_code.n_bits) == (n_cw, n_dec)
    assert chan.shape[1:] == (n_passes, cfg.n_sc * int(np.log2(cfg.constel_size))) and chan.shape[2] >= n_dec
    assert np.all(chan % 2 != 0) and np.abs(chan).max() <= 63
    np.testing.assert_array_equal((chan[:, :, :n_dec] < 0).sum(axis=2), rows[:, :, 0])
    assert np.all(rows[:, :, 3] <= rows[:, :, 2]) and np.all(rows[:, :, 2] <= n_cw)
    if totals:
        np.testing.assert_array_equal(rows.sum(axis=0), want, err_msg=f"{name}: the reference's totals per pass")


@pytest.mark.parametrize("name", sorted(CASES))
def test_turbo_rows_chan_z_and_counts(name):
    kw, iters, clean, key, n_passes, n_dec, n_cw, _ = CASES[name]
    ref = reference(name)
    assert_reference_conditions(name, *ref)
    cfg, ref_counts, ref_chan, ref_rows, ref_z = ref[:5]
    code = codes(key)[0]
    eng = engine_for(cfg, precision="f64")
    assert eng.coded_codewords(code) == n_cw
    err, bits, turbo, per, per_turbo, chan, z = eng.turbo(SEED, 0, N_TRIALS, iters, code, RHO_MAX, n_passes,
                                                          incl_clean=clean, per_trial=True, chan=True, z=True)
    kernel_ms, pass_ms = eng.kernel_ms, eng.decode_kernel_ms
    assert kernel_ms > 0 and pass_ms > 0 and eng.beam_kernel_ms == 0
    e_run, b_run, per_run = eng.run(SEED, 0, N_TRIALS, iters, incl_clean=clean, per_trial=True)
    assert eng.decode_kernel_ms == 0  # 0 after any other call
    print(name, eng.describe(), "counts", per.sum(0), "cells", turbo.tolist(), "kernel ms", kernel_ms, "pass loop ms",
          pass_ms, "max |z - oracle| / max |z|", np.abs(z - ref_z).max() / np.abs(ref_z).max())
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: turbo vs run")
    assert_counts_equal(per, ref_counts, f"{name}: turbo vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    # the received vectors: the oracle's, within the allowance the near-edge condition is built on
    assert z.shape == ref_z.shape == (N_TRIALS, cfg.n_sc) and z.dtype == np.complex128
    assert np.abs(z - ref_z).max() <= soft_ref.EPS_V * np.abs(ref_z).max()
    # the channel values of every pass: the reference's, byte for byte
    assert chan.dtype == np.int8 and chan.shape == ref_chan.shape
    np.testing.assert_array_equal(chan, ref_chan, err_msg=f"{name}: channel values")
    # per-trial rows: the reference's, cell for cell; totals: the row sums
    assert per_turbo.shape == ref_rows.shape == (N_TRIALS, n_passes, 4) and turbo.shape == (n_passes, 4)
    np.testing.assert_array_equal(per_turbo, ref_rows, err_msg=f"{name}: per-trial rows")
    np.testing.assert_array_equal(turbo, per_turbo.sum(axis=0))
    # pass 0 is the coded mode at CNC iteration 0, on the same engine
    _, _, coded, _, per_coded, chan_coded = eng.coded(SEED, 0, N_TRIALS, (0,), code, RHO_MAX, per_trial=True, chan=True)
    np.testing.assert_array_equal(per_turbo[:, 0], per_coded[:, 0])
    np.testing.assert_array_equal(chan[:, 0], chan_coded[:, 0])
    np.testing.assert_array_equal(turbo[0], coded[0])
    # without the optional outputs: the same rows (the streams then share one buffer)
    _, _, turbo2, _, per_turbo2 = eng.turbo(SEED, 0, N_TRIALS, iters, code, RHO_MAX, n_passes, incl_clean=clean,
                                            per_trial=True)
    np.testing.assert_array_equal(per_turbo2, per_turbo)
    np.testing.assert_array_equal(turbo2, turbo)
    eng.close()


def test_fixed_point_on_the_device():
    """The LoS case decodes every frame at pass 1 and has no tail: passes 2 and 3 are equal."""
    name = "f512_los-z64"
    kw, iters, clean, key, n_passes, _, _, _ = CASES[name]
    eng = engine_for(sim.SimConfig(**kw), precision="f64")
    _, _, _, _, rows, chan = eng.turbo(SEED, 0, N_TRIALS, iters, codes(key)[0], RHO_MAX, n_passes, per_trial=True, chan=True)
    eng.close()
    assert np.all(rows[:, 1, 1:] == 0)
    np.testing.assert_array_equal(rows[:, 2], rows[:, 3])
    np.testing.assert_array_equal(chan[:, 2], chan[:, 3])


def test_turbo_points_rows_and_repeatability():
    """The generic system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, one call,
    against per-point calls and the reference; a second identical call gives identical bits."""
    name = "f256_generic-z16"
    _, iters, clean, key, n_passes, _, _, _ = CASES[name]
    code = codes(key)[0]
    ibos, n_trials, first = (0.0, 3.0, 6.0), (5, 3, 4), (0, 16, 40)
    refs = [reference(name, ibo, f, n) for ibo, f, n in zip(ibos, first, n_trials)]
    for r in refs:
        assert_reference_conditions(name, *r, totals=False)
    eng = engine_for(refs[1][0], precision="f64")
    points = []
    for r in refs:
        e = engine_for(r[0], precision="f64")
        points.append(dict(e.point_kw))
        e.close()
    seeds = [SEED] * 3
    err, bits, turbo, per, per_turbo, chan, z = eng.turbo_points(points, seeds, first, n_trials, iters, code, RHO_MAX,
                                                                 n_passes, clean, True, chan=True, z=True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, clean, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "turbo_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[1] for r in refs]), "turbo_points vs oracle")
    np.testing.assert_array_equal(chan, np.concatenate([r[2] for r in refs]))
    np.testing.assert_array_equal(per_turbo, np.concatenate([r[3] for r in refs]))
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(3):
        own = slice(off[i], off[i + 1])
        np.testing.assert_array_equal(turbo[i], per_turbo[own].sum(axis=0))
        _, _, t1, _, pt1, c1, z1 = eng.turbo(seeds[i], first[i], n_trials[i], iters, code, RHO_MAX, n_passes, clean, True,
                                             point=points[i], chan=True, z=True)
        np.testing.assert_array_equal(pt1, per_turbo[own])
        np.testing.assert_array_equal(t1, turbo[i])
        np.testing.assert_array_equal(c1, chan[own])
        np.testing.assert_array_equal(z1, z[own])
    out2 = eng.turbo_points(points, seeds, first, n_trials, iters, code, RHO_MAX, n_passes, clean, True, chan=True, z=True)
    for a, b in zip(out2, (err, bits, turbo, per, per_turbo, chan, z)):
        np.testing.assert_array_equal(a, b)
    eng.close()


def test_turbo_totals_across_slices_and_launches(monkeypatch):
    """More trials than one reduction slice (4096), a call split into several launches by
    MIMO_MAX_LAUNCH_TRIALS and by a lowered MIMO_TURBO_BUFFER_BYTES: the totals are the per-trial
    rows' sums, and rows, channel values, vectors, counts and totals do not depend on the splitting."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0)
    code = codes("z16")[0]   # 768 bits: 8 codewords a trial
    eng = engine_for(cfg, precision="f64")
    n, n_passes = 4096 + 37, 3
    base = eng.turbo(7, 0, n, (0, 1), code, RHO_MAX, n_passes, per_trial=True, chan=True, z=True)
    err, _, turbo, per, pt, chan, z = base
    np.testing.assert_array_equal(turbo, pt.sum(axis=0))
    np.testing.assert_array_equal(err, per.sum(0))
    np.testing.assert_array_equal(turbo[0, 0], err[0])            # every position is decoded here
    np.testing.assert_array_equal((chan[:, 0] < 0).sum(axis=1), per[:, 0])
    np.testing.assert_array_equal((chan < 0).sum(axis=2), pt[:, :, 0])
    assert np.all(turbo[:, 3] <= turbo[:, 2]) and turbo[:, 2].max() <= 8 * n
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "1500")
    for a, b in zip(eng.turbo(7, 0, n, (0, 1), code, RHO_MAX, n_passes, per_trial=True, chan=True, z=True), base):
        np.testing.assert_array_equal(a, b)
    monkeypatch.delenv("MIMO_MAX_LAUNCH_TRIALS")
    # one trial takes 16 S + 3 * 768 + 768 = 5,120 B with the channel values asked for: 700 trials a launch
    monkeypatch.setenv("MIMO_TURBO_BUFFER_BYTES", str(5120 * 700))
    for a, b in zip(eng.turbo(7, 0, n, (0, 1), code, RHO_MAX, n_passes, per_trial=True, chan=True, z=True), base):
        np.testing.assert_array_equal(a, b)
    # ... and 16 S + 768 + 768 = 3,584 B without: the same rows from other launches
    out = eng.turbo(7, 0, n, (0, 1), code, RHO_MAX, n_passes, per_trial=True)
    np.testing.assert_array_equal(out[2], turbo)
    np.testing.assert_array_equal(out[4], pt)
    monkeypatch.setenv("MIMO_TURBO_BUFFER_BYTES", "3000")  # not one trial fits
    with pytest.raises(_engine.EngineError, match="MIMO_TURBO_BUFFER_BYTES"):
        eng.turbo(7, 0, 4, (0, 1), code, RHO_MAX, n_passes)
    eng.close()
