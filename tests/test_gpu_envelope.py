"""Envelope mode of the fused trial kernel (mimo_engine_envelope_points) on the GPU: the same counts
as the plain run and the oracle, the per-trial histograms of the instantaneous power at the PA
inputs and outputs equal to the oracle-built reference (tests/envelope_ref.py) cell for cell, the
fixed sums within the spectrum mode's bound, fixed-order totals, and the spectrum mode's Parseval
counterparts.

The histograms can be compared exactly because no sample of these cases lies within the allowed
amplitude error of a bin edge (``envelope_ref.near_edge == 0``, a condition on the inputs that every
case asserts on the reference before it looks at the device).
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import envelope_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import sim

pytestmark = pytest.mark.gpu

SEED = 7
N_TRIALS = 8
SNR64 = 25.0  # Es/N0 [dB] of the 64-QAM cases
NB = envelope_ref.ENV_BINS

# the spectrum test's cases, the smallest shapes that reach every code variant: (config, iters)
CASES = {
    # generic band, one wave
    "f256_generic": (dict(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                          channel="rayleigh"), (0, 1)),
    # aligned, 4 slots, closed-form channel; IBO 0 on purpose: every clipped sample at u = 1
    "f512_los": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", ibo_db=0.0, snr_db=SNR64,
                      channel="los"), (0, 1)),
    # the CSI instance: X from the estimate
    "f512_csi": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0,
                      channel="rayleigh", csi_eps=0.2), (0, 1)),
    # one-wave generic instance, cubic PA
    "f128_toi": (dict(n_ant=4, n_sc=64, n_fft=128, constel_size=16, pa="toi", ibo_db=5.0, snr_db=20.0,
                      channel="rayleigh"), (0, 1)),
    # wave-split FFT, T 256, the MCNC loop's re-transmissions
    "f2048_mcnc": (dict(n_ant=4, n_sc=1024, n_fft=2048, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                        channel="rayleigh", receiver="mcnc"), (0, 1, 2)),
    # 8 slots, 16-point team
    "f4096_rapp": (dict(n_ant=2, n_sc=2048, n_fft=4096, constel_size=64, pa="rapp", p_hardness=3.0, ibo_db=3.0,
                        snr_db=SNR64, channel="rayleigh"), (0, 1)),
    # split FFT, T 512
    "f8192": (dict(n_ant=2, n_sc=4096, n_fft=8192, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                   channel="rayleigh"), (0, 1)),
    # no PA: output = input
    "f256_nopa": (dict(n_ant=4, n_sc=128, n_fft=256, constel_size=64, pa="none", ibo_db=3.0, snr_db=SNR64,
                       channel="rayleigh"), (0,)),
}


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS, ref_scale=1.0):
    """(config, ref_pow, counts, rows, near-edge samples) of a case; ref_pow = ref_scale x the
    nominal mean sample power."""
    kw, iters = CASES[name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    ref_pow = ref_scale * envelope_ref.nominal_power(cfg)
    counts, rows, near = envelope_ref.reference(cfg, SEED, np.arange(first, first + n), iters, ref_pow)
    for a in (counts, rows):
        a.setflags(write=False)
    return cfg, ref_pow, counts, rows, near


def check_rows(label, rows_gpu, rows_ref):
    """Histograms exactly; Pin, Pout and C within 1e-12 Pin (spectrum_ref.row_bounds' rule for Ex and C)."""
    rows_gpu = np.asarray(rows_gpu)
    assert rows_gpu.shape == rows_ref.shape and np.all(np.isfinite(rows_gpu))
    np.testing.assert_array_equal(rows_gpu[:, :2 * NB], rows_ref[:, :2 * NB], err_msg=f"{label}: histograms")
    dev = np.abs(rows_gpu[:, 2 * NB:] - rows_ref[:, 2 * NB:])
    bound = 1e-12 * rows_ref[:, 2 * NB:2 * NB + 1]
    worst = (dev / bound).max(axis=0)
    print(f"ENVELOPE_RATIO case={label} fixed=" + ",".join(f"{v:.2e}" for v in worst))
    assert np.all(dev <= bound), f"{label}: a fixed sum deviates {worst.max():.3g} x its bound"


@pytest.mark.parametrize("name", sorted(CASES))
def test_envelope_rows_and_counts(name):
    cfg, ref_pow, ref_counts, ref_rows, near = reference(name)
    _, iters = CASES[name]
    # the condition on the inputs: no sample within the allowed error of an edge
    assert near == 0, f"{name}: {near} samples near a bin edge"
    n_samp = cfg.n_ant * cfg.n_fft
    assert np.all(ref_rows[:, :NB].sum(1) == n_samp) and np.all(ref_rows[:, NB:2 * NB].sum(1) == n_samp)
    eng = engine_for(cfg, precision="f64")
    err, bits, env, per, per_env = eng.envelope(SEED, 0, N_TRIALS, iters, ref_pow, per_trial=True)
    env_ms = eng.kernel_ms
    assert env_ms > 0  # mimo_engine_last_kernel_ms covers the mode's kernel
    e_run, b_run, per_run = eng.run(SEED, 0, N_TRIALS, iters, per_trial=True)
    print(name, eng.describe(), "counts", per.sum(0), "kernel ms", env_ms)
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: envelope vs run")
    assert_counts_equal(per, ref_counts, f"{name}: envelope vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert per_env.shape == ref_rows.shape == (N_TRIALS, 260)
    check_rows(name, per_env, ref_rows)
    # totals: the histogram cells exactly, the fixed sums in a fixed order
    np.testing.assert_array_equal(env[:2 * NB], per_env[:, :2 * NB].sum(0))
    np.testing.assert_allclose(env[2 * NB:], per_env[:, 2 * NB:].sum(0), rtol=1e-12, atol=1e-12 * env[2 * NB])
    if cfg.receiver == "mcnc":
        # the MCNC re-transmissions stay out: the rows of the same system under CNC, bit for bit
        eng_c = engine_for(dataclasses.replace(cfg, receiver="cnc"), precision="f64")
        _, _, env_c, _, per_env_c = eng_c.envelope(SEED, 0, N_TRIALS, iters, ref_pow, per_trial=True)
        np.testing.assert_array_equal(per_env_c, per_env)
        np.testing.assert_array_equal(env_c, env)
        eng_c.close()
    if cfg.pa == "none":
        np.testing.assert_array_equal(per_env[:, NB:2 * NB], per_env[:, :NB])
        np.testing.assert_array_equal(per_env[:, 2 * NB + 1], per_env[:, 2 * NB])
    # cross-mode: the same trials through the spectrum mode give Ex, sum psd and C (Parseval)
    _, _, _, _, per_spec = eng.spectrum(SEED, 0, N_TRIALS, iters, per_trial=True)
    f = cfg.n_fft
    pin = per_env[:, 2 * NB]
    assert np.all(np.abs(per_spec[:, f] - pin) <= 1e-12 * pin)
    assert np.all(np.abs(per_spec[:, :f].sum(1) - per_env[:, 2 * NB + 1]) <= 1e-12 * per_env[:, 2 * NB + 1])
    c_env = per_env[:, 2 * NB + 2] + 1j * per_env[:, 2 * NB + 3]
    c_spec = per_spec[:, f + 1] + 1j * per_spec[:, f + 2]
    assert np.all(np.abs(c_spec - c_env) <= 1e-12 * np.abs(c_env))
    eng.close()


def test_envelope_points_rows_and_repeatability():
    """Case 1's system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, one call."""
    name = "f256_generic"
    _, iters = CASES[name]
    ibos, n_trials, first = (0.0, 3.0, 6.0), (5, 3, 4), (0, 16, 40)
    refs = [reference(name, ibo, f, n) for ibo, f, n in zip(ibos, first, n_trials)]
    assert all(r[4] == 0 for r in refs)
    ref_pow = refs[1][1]
    assert all(r[1] == ref_pow for r in refs)  # the nominal mean does not depend on the IBO
    eng = engine_for(refs[1][0], precision="f64")
    points = []
    for r in refs:
        e = engine_for(r[0], precision="f64")
        points.append(dict(e.point_kw))
        e.close()
    seeds = [SEED] * 3
    err, bits, env, per, per_env = eng.envelope_points(points, seeds, first, n_trials, iters, ref_pow, per_trial=True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "envelope_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[2] for r in refs]), "envelope_points vs oracle")
    check_rows("multipoint", per_env, np.concatenate([r[3] for r in refs]))
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(3):
        own = per_env[off[i]:off[i + 1]]
        np.testing.assert_array_equal(env[i, :2 * NB], own[:, :2 * NB].sum(0))
        np.testing.assert_allclose(env[i, 2 * NB:], [math.fsum(c) for c in own[:, 2 * NB:].T], rtol=1e-12,
                                   atol=1e-12 * env[i, 2 * NB])
        # every point's rows and totals are those of a single-point call, bit for bit
        _, _, e1, _, pe1 = eng.envelope(seeds[i], first[i], n_trials[i], iters, ref_pow, per_trial=True,
                                        point=points[i])
        np.testing.assert_array_equal(pe1, own)
        np.testing.assert_array_equal(e1, env[i])
    # a second identical call: bit-identical totals and rows
    _, _, env2, _, per_env2 = eng.envelope_points(points, seeds, first, n_trials, iters, ref_pow, per_trial=True)
    np.testing.assert_array_equal(env2, env)
    np.testing.assert_array_equal(per_env2, per_env)
    eng.close()


def test_envelope_totals_across_slices_and_launches(monkeypatch):
    """More trials than one reduction slice (4096), and a call split into several launches
    (MIMO_MAX_LAUNCH_TRIALS): the totals are the per-trial rows' sums, the rows and counts do not
    depend on the splitting, and neither do the histogram totals."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64)
    ref_pow = envelope_ref.nominal_power(cfg)
    eng = engine_for(cfg, precision="f64")
    n = 4096 + 37
    err, _, env, per, pe = eng.envelope(SEED, 0, n, (0, 1), ref_pow, per_trial=True)
    np.testing.assert_array_equal(env[:2 * NB], pe[:, :2 * NB].sum(0))
    assert env[:NB].sum() == env[NB:2 * NB].sum() == n * 256
    np.testing.assert_allclose(env[2 * NB:], [math.fsum(c) for c in pe[:, 2 * NB:].T], rtol=1e-12,
                               atol=1e-12 * env[2 * NB])
    np.testing.assert_array_equal(err, per.sum(0))
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "1500")
    err3, _, env3, per3, pe3 = eng.envelope(SEED, 0, n, (0, 1), ref_pow, per_trial=True)
    np.testing.assert_array_equal(pe3, pe)
    np.testing.assert_array_equal(per3, per)
    np.testing.assert_array_equal(err3, err)
    np.testing.assert_array_equal(env3[:2 * NB], env[:2 * NB])
    np.testing.assert_allclose(env3[2 * NB:], env[2 * NB:], rtol=1e-12, atol=1e-12 * env[2 * NB])
    monkeypatch.delenv("MIMO_MAX_LAUNCH_TRIALS")
    # a repeated call: bit-identical
    _, _, env4, _, pe4 = eng.envelope(SEED, 0, n, (0, 1), ref_pow, per_trial=True)
    np.testing.assert_array_equal(env4, env)
    np.testing.assert_array_equal(pe4, pe)
    eng.close()


def test_twice_the_reference_power_moves_every_sample_by_eight_bins():
    """ref_pow doubled halves the bin scale exactly (a power of two), so every sample's bits >> 49
    fall by 8: the histograms of the first call moved down by 8 bins with the low end folded into
    bin 0 (the top bin is empty here, so nothing hides above it)."""
    name = "f256_generic"
    cfg, ref_pow, _, ref_rows, near = reference(name)
    _, ref_pow2, _, ref_rows2, near2 = reference(name, ref_scale=2.0)
    assert near == 0 and near2 == 0 and ref_pow2 == 2.0 * ref_pow
    assert np.all(ref_rows[:, NB - 1] == 0) and np.all(ref_rows[:, 2 * NB - 1] == 0)
    _, iters = CASES[name]
    eng = engine_for(cfg, precision="f64")
    _, _, _, _, pe1 = eng.envelope(SEED, 0, N_TRIALS, iters, ref_pow, per_trial=True)
    _, _, _, _, pe2 = eng.envelope(SEED, 0, N_TRIALS, iters, ref_pow2, per_trial=True)
    eng.close()

    def moved(h):
        out = np.zeros_like(h)
        out[:, 0] = h[:, :9].sum(1)
        out[:, 1:NB - 8] = h[:, 9:]
        return out

    np.testing.assert_array_equal(pe2[:, :NB], moved(pe1[:, :NB]))
    np.testing.assert_array_equal(pe2[:, NB:2 * NB], moved(pe1[:, NB:2 * NB]))
    np.testing.assert_array_equal(pe2[:, 2 * NB:], pe1[:, 2 * NB:])  # the fixed sums do not read ref_pow
    check_rows("ref_pow x 2", pe2, ref_rows2)


def test_link_envelope_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    import _engine
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM, soft limiter at IBO 1
    pp = link.point_params()
    nominal = pp["sat_pow"] / 10 ** (pp["ibo_db"] / 10)
    assert link.nominal_sample_power() == nominal
    link.set_snr(14.0)
    st = link.envelope(True, [11, 22, 33], N_TRIALS)
    assert (st.n_ant, st.n_fft, st.n_trials, st.ref_pow) == (8, 128, N_TRIALS, nominal)
    eng = link.engine()
    _, _, env, _, _ = eng.envelope(_seed64([11, 22, 33]), 0, N_TRIALS, [0], nominal, point=link.point_params())
    np.testing.assert_array_equal(st.row, env)
    assert st.n_samples == N_TRIALS * 8 * 128 == st.hist_in.sum() == st.hist_out.sum()
    ref = _engine.EnvelopeStats(env, 8, 128, N_TRIALS, nominal)
    assert st.efficiency == ref.efficiency and st.gain == ref.gain and st.level_db(1e-2) == ref.level_db(1e-2)
    # 0 dB is the mean, and the limiter's clip level reads as the IBO (1 dB): nothing leaves above its bin
    assert abs(st.mean_in_db) < 0.3
    b = int(envelope_ref.bin_of(np.array([10.0 ** 0.1]), 1.0)[0])
    assert st.hist_in[b + 1:].sum() > 0 and np.all(st.hist_out[b + 1:] == 0)
    assert st.level_db(0.0, "out") == st.edges_db[b]
    assert 0.5 < st.efficiency < 1.0 and 0.5 < abs(st.gain) < 1.0
    # an explicit ref_pow, and envelope_points at two IBOs: point 0 is the call above
    st2 = link.envelope(True, [11, 22, 33], N_TRIALS, ref_pow=2.0 * nominal)
    assert st2.ref_pow == 2.0 * nominal and st2.hist_in[0] >= st.hist_in[0]
    np.testing.assert_array_equal(st2.row[256:], st.row[256:])
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.envelope_points(True, [[11, 22, 33], [5]], [p0, p1], N_TRIALS)
    np.testing.assert_array_equal(both[0].row, st.row)
    assert both[1].ref_pow == nominal and both[1].efficiency > both[0].efficiency  # more back-off, less clipped
