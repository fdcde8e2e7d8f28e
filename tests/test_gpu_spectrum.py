"""Spectrum mode of the fused trial kernel (mimo_engine_spectrum_points) on the GPU: the same
counts as the plain run and the oracle, per-trial PSD rows per FFT bin against the oracle-built
reference (tests/spectrum_ref.py) within a bound derived from the allowed error on a chain
output, fixed-order totals, and the physics the radiated spectrum must show.

Measured worst deviation-to-bound ratios per case: profiles/r09/spectrum/accuracy.md.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import spectrum_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import refmath as rm
from oracle import sim

pytestmark = pytest.mark.gpu

SEED = 7
N_TRIALS = 8
SNR64 = 25.0  # Es/N0 [dB] of the 64-QAM cases

# the smallest shapes that reach every variant of the spectrum code: (config, iters)
CASES = {
    # generic band, one wave
    "f256_generic": (dict(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                          channel="rayleigh"), (0, 1)),
    # aligned, 4 slots, closed-form channel
    "f512_los": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
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
    # split FFT, T 512: the permuted frequency thread
    "f8192": (dict(n_ant=2, n_sc=4096, n_fft=8192, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                   channel="rayleigh"), (0, 1)),
    # no PA: nothing out of band
    "f256_nopa": (dict(n_ant=4, n_sc=128, n_fft=256, constel_size=64, pa="none", ibo_db=3.0, snr_db=SNR64,
                       channel="rayleigh"), (0,)),
}


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS):
    kw, iters = CASES[name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    counts, rows = spectrum_ref.reference_rows(cfg, SEED, np.arange(first, first + n), iters)
    for a in (counts, rows):
        a.setflags(write=False)
    return cfg, counts, rows


def worst_ratio(label, rows_gpu, rows_ref):
    dev = np.abs(np.asarray(rows_gpu) - rows_ref)
    bound = spectrum_ref.row_bounds(rows_ref)
    ratio = dev / bound
    worst = float(ratio.max())
    col = int(np.unravel_index(np.argmax(ratio), ratio.shape)[1])
    f = rows_ref.shape[1] - spectrum_ref.SPEC_FIXED
    print(f"SPECTRUM_RATIO case={label} worst={worst:.3e} column={col} psd={ratio[:, :f].max():.2e} "
          "fixed=" + ",".join(f"{v:.2e}" for v in ratio[:, f:].max(axis=0)))
    return worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_spectrum_rows_and_counts(name):
    cfg, ref_counts, ref_rows = reference(name)
    _, iters = CASES[name]
    f = cfg.n_fft
    eng = engine_for(cfg, precision="f64")
    err, bits, spec, per, per_spec = eng.spectrum(SEED, 0, N_TRIALS, iters, per_trial=True)
    e_run, b_run, per_run = eng.run(SEED, 0, N_TRIALS, iters, per_trial=True)
    print(name, eng.describe(), "counts", per.sum(0))
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: spectrum vs run")
    assert_counts_equal(per, ref_counts, f"{name}: spectrum vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert per_spec.shape == ref_rows.shape == (N_TRIALS, f + 3)
    assert np.all(np.isfinite(per_spec))
    worst = worst_ratio(name, per_spec, ref_rows)
    assert worst <= 1.0, f"{name}: per-trial row deviates {worst:.3g} x its bound"
    np.testing.assert_allclose(spec, per_spec.sum(0), rtol=1e-12, atol=0)
    if cfg.receiver == "mcnc":
        # the MCNC re-transmissions stay out: the rows of the same system under CNC, bit for bit
        eng_c = engine_for(dataclasses.replace(cfg, receiver="cnc"), precision="f64")
        _, _, spec_c, _, per_spec_c = eng_c.spectrum(SEED, 0, N_TRIALS, iters, per_trial=True)
        np.testing.assert_array_equal(per_spec_c, per_spec)
        np.testing.assert_array_equal(spec_c, spec)
        eng_c.close()
    if cfg.pa == "none":
        oob = np.ones(f, bool)
        oob[rm.inband_bins(f, cfg.n_sc)] = False
        assert ref_rows[:, :f][:, oob].max() < 1e-29
        bound = spectrum_ref.row_bounds(ref_rows)[:, :f]
        assert np.all(per_spec[:, :f][:, oob] <= bound[:, oob])
        ex = per_spec[:, f]
        assert np.all(np.abs(per_spec[:, :f].sum(1) - ex) <= 1e-12 * ex)
    eng.close()


def test_spectrum_points_rows_and_repeatability():
    """Case 1's system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, one call."""
    name = "f256_generic"
    _, iters = CASES[name]
    ibos, n_trials, first = (0.0, 3.0, 6.0), (5, 3, 4), (0, 16, 40)
    refs = [reference(name, ibo, f, n) for ibo, f, n in zip(ibos, first, n_trials)]
    eng = engine_for(refs[1][0], precision="f64")
    points = []
    for r in refs:
        e = engine_for(r[0], precision="f64")
        points.append(dict(e.point_kw))
        e.close()
    seeds = [SEED] * 3
    err, bits, spec, per, per_spec = eng.spectrum_points(points, seeds, first, n_trials, iters, per_trial=True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "spectrum_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[1] for r in refs]), "spectrum_points vs oracle")
    worst = worst_ratio("multipoint", per_spec, np.concatenate([r[2] for r in refs]))
    assert worst <= 1.0
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(3):
        own = per_spec[off[i]:off[i + 1]]
        np.testing.assert_allclose(spec[i], [math.fsum(c) for c in own.T], rtol=1e-12, atol=0)
        # every point's rows are those of a single-point call, bit for bit
        _, _, s1, _, ps1 = eng.spectrum(seeds[i], first[i], n_trials[i], iters, per_trial=True, point=points[i])
        np.testing.assert_array_equal(ps1, own)
        np.testing.assert_allclose(s1, spec[i], rtol=1e-12, atol=0)
    # a second identical call: bit-identical totals and rows
    _, _, spec2, _, per_spec2 = eng.spectrum_points(points, seeds, first, n_trials, iters, per_trial=True)
    np.testing.assert_array_equal(spec2, spec)
    np.testing.assert_array_equal(per_spec2, per_spec)
    eng.close()


def test_spectrum_totals_across_slices_and_launches(monkeypatch):
    """More trials than one reduction slice (4096), and a call split into several launches
    (MIMO_MAX_LAUNCH_TRIALS): the totals are the per-trial rows' sums, the rows and counts do not
    depend on the splitting."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64)
    eng = engine_for(cfg, precision="f64")
    n = 4096 + 37
    err, _, spec, per, ps = eng.spectrum(SEED, 0, n, (0, 1), per_trial=True)
    np.testing.assert_allclose(spec, [math.fsum(c) for c in ps.T], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(err, per.sum(0))
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "1500")
    err3, _, spec3, per3, ps3 = eng.spectrum(SEED, 0, n, (0, 1), per_trial=True)
    np.testing.assert_array_equal(ps3, ps)
    np.testing.assert_array_equal(per3, per)
    np.testing.assert_array_equal(err3, err)
    np.testing.assert_allclose(spec3, spec, rtol=1e-12, atol=0)
    np.testing.assert_allclose(spec3, [math.fsum(c) for c in ps3.T], rtol=1e-12, atol=0)
    eng.close()


def test_link_spectrum_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM
    link.set_snr(14.0)
    st = link.spectrum(True, [11, 22, 33], N_TRIALS)
    eng = link.engine()
    _, _, spec, _, _ = eng.spectrum(_seed64([11, 22, 33]), 0, N_TRIALS, [0], point=link.point_params())
    np.testing.assert_array_equal(st.row, spec)
    assert (st.n_fft, st.n_sub_carr, st.n_trials) == (128, 64, N_TRIALS)
    import _engine
    ref = _engine.SpectrumStats(spec, 64)
    assert st.oob_ratio_db == ref.oob_ratio_db and st.gain == ref.gain and st.efficiency == ref.efficiency
    assert -40.0 < st.oob_ratio_db < -5.0 and 0.5 < st.efficiency < 1.0
    # through spectrum_points at two IBOs: point 0 is the call above
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.spectrum_points(True, [[11, 22, 33], [5]], [p0, p1], N_TRIALS)
    np.testing.assert_array_equal(both[0].row, st.row)
    assert both[1].oob_ratio_db < both[0].oob_ratio_db  # more back-off, less regrowth


# ---------------------------------------------------------------- physics of the radiated spectrum
PHYS = dict(n_ant=4, n_sc=128, n_fft=256, constel_size=64, pa="softlim", snr_db=SNR64, channel="rayleigh")
PHYS_TRIALS = 32
PHYS_IBOS = (0.0, 3.0, 6.0)


@functools.lru_cache(maxsize=None)
def pooled_spectrum(ibo):
    """(oracle, GPU) pooled SpectrumStats over trials 0-31, seed 7."""
    import _engine
    cfg = sim.SimConfig(ibo_db=ibo, **PHYS)
    _, rows = spectrum_ref.reference_rows(cfg, SEED, np.arange(PHYS_TRIALS), (0,))
    ref = _engine.SpectrumStats(rows.sum(0), cfg.n_sc, PHYS_TRIALS)
    eng = engine_for(cfg, precision="f64")
    _, _, spec, _, _ = eng.spectrum(SEED, 0, PHYS_TRIALS, (0,))
    eng.close()
    gpu = _engine.SpectrumStats(spec, cfg.n_sc, PHYS_TRIALS)
    print(f"SPECTRUM_PHYS ibo={ibo}: oracle efficiency {ref.efficiency:.6f} |gain| {abs(ref.gain):.6f} "
          f"oob {ref.oob_ratio_db:.4f} dB; gpu {gpu.efficiency:.6f} {abs(gpu.gain):.6f} {gpu.oob_ratio_db:.4f} dB")
    return ref, gpu


@pytest.mark.parametrize("ibo", PHYS_IBOS)
def test_pooled_gpu_figures_equal_the_reference(ibo):
    ref, gpu = pooled_spectrum(ibo)
    assert abs(gpu.efficiency - ref.efficiency) <= 1e-9 * ref.efficiency
    assert abs(abs(gpu.gain) - abs(ref.gain)) <= 1e-9 * abs(ref.gain)
    assert abs(gpu.oob_ratio_db - ref.oob_ratio_db) <= 1e-9


@pytest.mark.parametrize("ibo", PHYS_IBOS)
def test_efficiency_and_gain_follow_the_soft_limiter_formulas(ibo):
    """Radiated over input power of a soft limiter on a Gaussian signal is 1 - exp(-gamma^2),
    gamma^2 = 10^(IBO/10); its Bussgang gain is Modem.calc_alpha(IBO).  Conditions on the reference."""
    ref, _ = pooled_spectrum(ibo)
    eff = 1.0 - math.exp(-10.0 ** (ibo / 10.0))
    assert abs(ref.efficiency - eff) <= 0.015 * eff, (ibo, ref.efficiency, eff)
    alpha = float(rm.calc_alpha(ibo))
    assert abs(abs(ref.gain) - alpha) <= 0.015 * alpha, (ibo, abs(ref.gain), alpha)


def test_oob_share_falls_with_back_off():
    oob = [pooled_spectrum(ibo)[0].oob_ratio_db for ibo in PHYS_IBOS]
    assert oob[0] > oob[1] > oob[2], oob
