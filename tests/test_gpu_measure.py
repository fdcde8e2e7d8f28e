"""Measure mode of the fused trial kernel (mimo_engine_measure_points) on the GPU: the same
counts as the plain run and the oracle, per-trial power sums against the oracle-built
reference (tests/measure_ref.py) within a bound derived from the allowed error on z, fixed-order
totals, and the physics the in-band SDR must show.

Measured worst deviation-to-bound ratios per case: profiles/r08/measure/accuracy.md.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import measure_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import sim

pytestmark = pytest.mark.gpu

SEED = 7
N_TRIALS = 8
SNR64 = 25.0  # Es/N0 [dB] of the 64-QAM cases

# the smallest shapes that reach every variant of the measure code: (config, iters, incl_clean)
CASES = {
    # generic band, one wave, partial valid_mask; the clean index
    "f256_generic_clean": (dict(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0,
                                snr_db=SNR64, channel="rayleigh"), (0, 1, 3), True),
    # aligned, 4 slots, closed-form channel
    "f512_los": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                      channel="los"), (0, 2), False),
    # the CSI instance, channel with its FSPL factor
    "f512_csi": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0,
                      channel="rayleigh", csi_eps=0.2), (0, 1), False),
    # wave-split FFT, T 256, the MCNC loop
    "f2048_mcnc": (dict(n_ant=4, n_sc=1024, n_fft=2048, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                        channel="rayleigh", receiver="mcnc"), (0, 1, 2), False),
    # 8 slots, 16-point team
    "f4096_rapp": (dict(n_ant=2, n_sc=2048, n_fft=4096, constel_size=64, pa="rapp", p_hardness=3.0, ibo_db=3.0,
                        snr_db=SNR64, channel="rayleigh"), (0, 1), False),
    # split FFT, T 512
    "f8192": (dict(n_ant=2, n_sc=4096, n_fft=8192, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                   channel="rayleigh"), (0, 1), False),
}


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS):
    kw, iters, clean = CASES[name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    counts, rows, ez = measure_ref.reference_rows(cfg, SEED, np.arange(first, first + n), iters, clean)
    for a in (counts, rows, ez):
        a.setflags(write=False)
    return cfg, counts, rows, ez


def worst_ratio(label, rows_gpu, rows_ref, ez):
    dev = np.abs(np.asarray(rows_gpu) - rows_ref)
    bound = measure_ref.row_bounds(rows_ref, ez)
    ratio = dev / bound
    worst = float(ratio.max())
    col = int(np.unravel_index(np.argmax(ratio), ratio.shape)[1])
    print(f"MEASURE_RATIO case={label} worst={worst:.3e} column={col} per_column="
          + ",".join(f"{v:.2e}" for v in ratio.max(axis=0)))
    return worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_measure_rows_and_counts(name):
    cfg, ref_counts, ref_rows, ez = reference(name)
    _, iters, clean = CASES[name]
    eng = engine_for(cfg, precision="f64")
    err, bits, meas, per, per_meas = eng.measure(SEED, 0, N_TRIALS, iters, clean, per_trial=True)
    e_run, b_run, per_run = eng.run(SEED, 0, N_TRIALS, iters, clean, per_trial=True)
    print(name, eng.describe(), "counts", per.sum(0))
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: measure vs run")
    assert_counts_equal(per, ref_counts, f"{name}: measure vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert per_meas.shape == ref_rows.shape == (N_TRIALS, measure_ref.MEAS_FIXED + len(iters) + int(clean))
    assert np.all(np.isfinite(per_meas))
    worst = worst_ratio(name, per_meas, ref_rows, ez)
    assert worst <= 1.0, f"{name}: per-trial row deviates {worst:.3g} x its bound"
    np.testing.assert_allclose(meas, per_meas.sum(0), rtol=1e-12, atol=0)
    eng.close()


def test_measure_points_totals_rows_and_repeatability():
    """Case 1's system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, one call."""
    name = "f256_generic_clean"
    _, iters, clean = CASES[name]
    ibos, n_trials, first = (0.0, 3.0, 6.0), (5, 3, 4), (0, 16, 40)
    refs = [reference(name, ibo, f, n) for ibo, f, n in zip(ibos, first, n_trials)]
    eng = engine_for(refs[1][0], precision="f64")
    points = []
    for r in refs:
        e = engine_for(r[0], precision="f64")
        points.append(dict(e.point_kw))
        e.close()
    seeds = [SEED] * 3
    err, bits, meas, per, per_meas = eng.measure_points(points, seeds, first, n_trials, iters, clean, per_trial=True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, clean, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "measure_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[1] for r in refs]), "measure_points vs oracle")
    worst = worst_ratio("multipoint", per_meas, np.concatenate([r[2] for r in refs]),
                        np.concatenate([r[3] for r in refs]))
    assert worst <= 1.0
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(3):
        own = per_meas[off[i]:off[i + 1]]
        # every point's totals are the sum of its own per-trial rows
        np.testing.assert_allclose(meas[i], [math.fsum(c) for c in own.T], rtol=1e-12, atol=0)
        # ... and its rows those of a single-point call, bit for bit
        _, _, m1, _, pm1 = eng.measure(seeds[i], first[i], n_trials[i], iters, clean, per_trial=True, point=points[i])
        np.testing.assert_array_equal(pm1, own)
        np.testing.assert_allclose(m1, meas[i], rtol=1e-12, atol=0)
    # a second identical call: bit-identical totals
    _, _, meas2, _, per_meas2 = eng.measure_points(points, seeds, first, n_trials, iters, clean, per_trial=True)
    np.testing.assert_array_equal(meas2, meas)
    np.testing.assert_array_equal(per_meas2, per_meas)
    eng.close()


def test_measure_totals_across_slices_and_launches(monkeypatch):
    """More trials than one reduction slice (4096), and a call split into several launches
    (MIMO_MAX_LAUNCH_TRIALS): the totals are the per-trial rows' sums and repeat bit for bit,
    the rows do not depend on the splitting."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64)
    eng = engine_for(cfg, precision="f64")
    n = 4096 + 37
    err, _, meas, per, pm = eng.measure(SEED, 0, n, (0, 1), per_trial=True)
    np.testing.assert_allclose(meas, [math.fsum(c) for c in pm.T], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(err, per.sum(0))
    _, _, meas2, _, _ = eng.measure(SEED, 0, n, (0, 1))
    np.testing.assert_array_equal(meas2, meas)
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "1500")
    err3, _, meas3, per3, pm3 = eng.measure(SEED, 0, n, (0, 1), per_trial=True)
    np.testing.assert_array_equal(pm3, pm)
    np.testing.assert_array_equal(per3, per)
    np.testing.assert_array_equal(err3, err)
    np.testing.assert_allclose(meas3, meas, rtol=1e-12, atol=0)
    eng.close()


def test_link_measure_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM
    link.set_snr(14.0)
    st = link.measure(True, True, np.array([1, 0]), [11, 22, 33], N_TRIALS)
    eng = link.engine()
    err, bits, meas, _, _ = eng.measure(_seed64([11, 22, 33]), 0, N_TRIALS, [0, 1], True, point=link.point_params())
    np.testing.assert_array_equal(st.row, meas)
    np.testing.assert_array_equal(st.err, err)
    np.testing.assert_array_equal(st.bits, bits)
    import _engine
    ref = _engine.SignalStats(meas, err, bits)
    assert st.sdr_db == ref.sdr_db and st.slicer_sdr_db == ref.slicer_sdr_db and st.gain == ref.gain
    np.testing.assert_array_equal(st.sndr_db, ref.sndr_db)
    assert st.row.size == 5 + 3 and np.all(st.bits == N_TRIALS * 64 * 4)
    # the current point is what measure() ran: simulate's counters see the same trials
    e_run, _, _ = eng.run(_seed64([11, 22, 33]), 0, N_TRIALS, [0, 1], True)
    np.testing.assert_array_equal(st.err, e_run)
    # through measure_points at two IBOs: point 0 is the call above
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.measure_points(True, True, [0, 1], [[11, 22, 33], [5]], [p0, p1], N_TRIALS)
    np.testing.assert_array_equal(both[0].row, st.row)
    assert both[1].sdr_db > both[0].sdr_db  # more back-off, less distortion


# ---------------------------------------------------------------- physics of the in-band SDR
PHYS = dict(n_sc=128, n_fft=256, constel_size=64, pa="softlim", snr_db=SNR64)
PHYS_TRIALS = 32


@functools.lru_cache(maxsize=None)
def physics_cfg(kind, ibo):
    if kind == "siso_flat":
        return sim.SimConfig(n_ant=1, ibo_db=ibo, channel="table", table_h=np.ones((1, PHYS["n_fft"]), np.complex128),
                             reroll=False, **PHYS)
    return sim.SimConfig(n_ant=16, ibo_db=ibo, channel=kind, **PHYS)


@functools.lru_cache(maxsize=None)
def pooled_sdr(kind, ibo):
    """(oracle, GPU) pooled in-band SDR [dB] over trials 0-31, seed 7; the GPU's within 1e-9 dB."""
    import _engine
    cfg = physics_cfg(kind, ibo)
    _, rows, _ = measure_ref.reference_rows(cfg, SEED, np.arange(PHYS_TRIALS), (0,))
    ref = _engine.SignalStats(rows.sum(0)).sdr_db
    eng = engine_for(cfg, precision="f64")
    err, bits, meas, _, _ = eng.measure(SEED, 0, PHYS_TRIALS, (0,))
    eng.close()
    gpu = _engine.SignalStats(meas, err, bits).sdr_db
    print(f"MEASURE_SDR {kind} ibo={ibo}: oracle {ref:.6f} dB, gpu {gpu:.6f} dB, diff {gpu - ref:.2e}")
    assert abs(gpu - ref) <= 1e-9, (kind, ibo, gpu, ref)
    return ref, gpu


@pytest.mark.parametrize("ibo", [0.0, 3.0, 6.0])
def test_siso_flat_sdr_between_total_and_inband_limits(ibo):
    """Only part of the clipping distortion falls in band: the in-band SDR lies strictly between
    the soft limiter's total-power SDR and that plus 10 log10(F / S)."""
    from sweep import soft_limiter_sdr
    lo = 10 * np.log10(float(soft_limiter_sdr(ibo)))
    hi = lo + 10 * np.log10(PHYS["n_fft"] / PHYS["n_sc"])
    for v in pooled_sdr("siso_flat", ibo):
        assert lo < v < hi, (ibo, lo, v, hi)


def test_los_array_sdr_equals_siso():
    """Over LoS the distortion is beamformed with the signal: 16 antennas gain nothing."""
    for v, s in zip(pooled_sdr("los", 3.0), pooled_sdr("siso_flat", 3.0)):
        assert abs(v - s) <= 1.0, (v, s)


def test_rayleigh_array_sdr_gains_the_array_factor():
    """Over i.i.d. Rayleigh the distortion is not beamformed: about 10 log10(A) better."""
    for v, s in zip(pooled_sdr("rayleigh", 3.0), pooled_sdr("siso_flat", 3.0)):
        assert abs(v - s - 10 * np.log10(16)) <= 1.5, (v, s)
