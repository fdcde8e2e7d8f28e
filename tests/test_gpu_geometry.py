"""The fused trial kernel off the default geometry (tests/geometry_cases.py): a spread-out array
close to a user whose x differs from its y, on a band 60 % of the centre frequency wide, so that
``ant_rel``, ``f_rel`` and the centre of the y jitter -- all within a percent of 1, or
indistinguishable, everywhere else in the suite -- decide the counts.

* counts of all 16 cases in both precisions against the float64 oracle: float64 exact; float32 by
  the project's float32 criterion (that of test_two_path_null_vs_oracle)
* float64 measure, spectrum and beam rows on the same geometry, bounds of the three ``*_ref.py``
* three reference-style links (planar, circular and linear array) through ``Link.engine()``

tests/test_geometry_cases.py shows on the CPU that every mutant of the oracle (antennas reversed
or equal, attenuation flat in frequency, y jittered around ``rx_pos[1]``, the noise power's 1 / f^2
weight dropped) moves more than a quarter of each case's entries.  Measured agreement and
row-to-bound ratios: profiles/r13/geometry/README.md.
"""
import functools

import numpy as np
import pytest

import beam_ref
import geometry_cases as gc
import measure_ref
import spectrum_ref
from gpu_util import PRECISIONS, assert_counts_equal, count_agreement, engine_for
from oracle import refmath as rm
from oracle import sim

pytestmark = pytest.mark.gpu

ITERS = list(gc.ITERS)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("num", gc.CASE_NUMBERS, ids=gc.case_id)
def test_counts_vs_oracle(num, prec):
    """float64: per-trial counts EXACTLY the oracle's, totals their column sums, bit counts right.
    float32 (unequal antennas and a wide band have no earlier float32 run): at least 95 % of the
    entries equal, none off by more than 2 bits, totals within 2 % + 4."""
    cfg, trials = gc.case_config(num)
    ref = gc.reference(num)
    eng = engine_for(cfg, precision=prec)
    err, bits, per = eng.run(gc.SEED, 0, len(trials), ITERS, True, per_trial=True)
    desc = eng.describe()
    eng.close()
    per = np.asarray(per, np.int64)
    agree = count_agreement(per, ref)
    print(f"GEOMETRY_AGREE case={gc.case_id(num)} prec={prec} [{desc}] agreement={agree:.4f} "
          f"differ={int((per != ref).sum())}/{ref.size} max_off={int(np.abs(per - ref).max())} "
          f"gpu={per.sum(0).tolist()} oracle={ref.sum(0).tolist()}")
    assert desc.endswith(prec), desc
    np.testing.assert_array_equal(err, per.sum(0))
    assert all(int(b) == len(trials) * cfg.n_sc * int(np.log2(cfg.constel_size)) for b in bits)
    if prec == "f64":
        assert_counts_equal(per, ref, f"{gc.case_id(num)} f64")
    else:
        assert agree >= 0.95, agree
        assert np.abs(per - ref).max() <= 2
        tot, tot_ref = per.sum(0).astype(float), ref.sum(0).astype(float)
        assert np.all(np.abs(tot - tot_ref) <= 0.02 * tot_ref + 4), (tot, tot_ref)


def test_the_distance_rule_keeps_every_run_that_divides_by_none():
    """The run calls refuse an antenna at the user, and for LoS / two-path at the jitter's centre
    (tests/test_abi.py).  What stays: a Rayleigh engine with an antenna at (rx_pos[0], rx_pos[0],
    rx_pos[2]) -- it reads rx_pos alone -- and a table engine with the user on an antenna -- it
    reads no position.  Both run, float64 counts EXACTLY the oracle's."""
    cfg, _ = gc.case_config(4)
    cfg.tx_pos = cfg.tx_pos.copy()
    cfg.tx_pos[3] = (gc.RX_POS[0], gc.RX_POS[0], gc.RX_POS[2])
    rng = np.random.default_rng(13)
    h = (rng.standard_normal((4, 128)) + 1j * rng.standard_normal((4, 128))) * 1e-6
    tab = sim.SimConfig(4, 64, 128, 16, ibo_db=2.0, snr_db=12.0, channel="table", table_h=h,
                        tx_pos=gc.sparse_positions(4), rx_pos=tuple(gc.sparse_positions(4)[2]))
    for label, c in (("rayleigh", cfg), ("table", tab)):
        ref = sim.run_trials(c, gc.SEED, np.arange(8), iters=ITERS, incl_clean=True)
        eng = engine_for(c, precision="f64")
        _, _, per = eng.run(gc.SEED, 0, 8, ITERS, True, per_trial=True)
        eng.close()
        print("GEOMETRY_DISTANCE_EDGE", label, per.sum(0).tolist(), ref.sum(0).tolist())
        assert ref.sum() > 0
        assert_counts_equal(per, ref, f"distance edge {label}")


# ---------------------------------------------------------------- float64 rows on the same geometry
N_ROWS = 8  # trials of the row tests: the first 8 of the case (all 6 of case 13)


def _row_trials(num):
    cfg, trials = gc.case_config(num)
    return cfg, trials[:N_ROWS]


@functools.lru_cache(maxsize=None)
def measure_reference(num):
    cfg, trials = _row_trials(num)
    out = measure_ref.reference_rows(cfg, gc.SEED, trials, ITERS, True, chunk=4)
    for a in out:
        a.setflags(write=False)
    return out


# LoS on generic slots; the CSI instance; two-path; MCNC at F 4096 (two-path too)
@pytest.mark.parametrize("num", [2, 5, 7, 13], ids=gc.case_id)
def test_measure_rows(num):
    """Per-trial measure rows within measure_ref.row_bounds, unchanged: 1e-13 relative on z."""
    cfg, trials = _row_trials(num)
    ref_counts, ref_rows, ez = measure_reference(num)
    np.testing.assert_array_equal(ref_counts, gc.reference(num)[:len(trials)])
    eng = engine_for(cfg, precision="f64")
    err, bits, meas, per, per_meas = eng.measure(gc.SEED, 0, len(trials), ITERS, True, per_trial=True)
    eng.close()
    assert_counts_equal(per, ref_counts, f"{gc.case_id(num)}: measure vs oracle")
    assert per_meas.shape == ref_rows.shape == (len(trials), measure_ref.MEAS_FIXED + len(ITERS) + 1)
    assert np.all(np.isfinite(per_meas))
    ratio = np.abs(per_meas - ref_rows) / measure_ref.row_bounds(ref_rows, ez)
    print(f"GEOMETRY_MEASURE_RATIO case={gc.case_id(num)} worst={ratio.max():.3e} per_column="
          + ",".join(f"{v:.2e}" for v in ratio.max(axis=0)))
    assert ratio.max() <= 1.0, f"{gc.case_id(num)}: a measure row deviates {ratio.max():.3g} x its bound"
    np.testing.assert_allclose(meas, per_meas.sum(0), rtol=1e-12, atol=0)


@functools.lru_cache(maxsize=None)
def spectrum_reference(num):
    cfg, trials = _row_trials(num)
    out = spectrum_ref.reference_rows(cfg, gc.SEED, trials, ITERS, True, chunk=4)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("num", [4, 10], ids=gc.case_id)
def test_spectrum_rows(num):
    """Per-trial spectrum rows within spectrum_ref.row_bounds, unchanged."""
    cfg, trials = _row_trials(num)
    ref_counts, ref_rows = spectrum_reference(num)
    np.testing.assert_array_equal(ref_counts, gc.reference(num)[:len(trials)])
    eng = engine_for(cfg, precision="f64")
    err, bits, spec, per, per_spec = eng.spectrum(gc.SEED, 0, len(trials), ITERS, True, per_trial=True)
    eng.close()
    assert_counts_equal(per, ref_counts, f"{gc.case_id(num)}: spectrum vs oracle")
    assert per_spec.shape == ref_rows.shape == (len(trials), cfg.n_fft + spectrum_ref.SPEC_FIXED)
    assert np.all(np.isfinite(per_spec))
    ratio = np.abs(per_spec - ref_rows) / spectrum_ref.row_bounds(ref_rows)
    f = cfg.n_fft
    print(f"GEOMETRY_SPECTRUM_RATIO case={gc.case_id(num)} worst={ratio.max():.3e} psd={ratio[:, :f].max():.2e} fixed="
          + ",".join(f"{v:.2e}" for v in ratio[:, f:].max(axis=0)))
    assert ratio.max() <= 1.0, f"{gc.case_id(num)}: a spectrum row deviates {ratio.max():.3g} x its bound"
    np.testing.assert_allclose(spec, per_spec.sum(0), rtol=1e-12, atol=0)


BEAM_CASE = 4


def beam_probes():
    """9 probes, an odd list (the last wave of the beamforming kernel half filled): seven on a 30 m
    circle at the user's height, one 3 m from antenna 0 (every antenna with a visibly different
    1 / d), one 50 km away (1.9e4 cycles through the phase reduction at 100 MHz; beam_ref.eps_g
    scales with d f / c)."""
    from utilities import circle_probes
    near = gc.sparse_positions(8)[0] + [0.0, 3.0, 0.0]
    return np.concatenate([circle_probes(np.arange(0.0, 181.0, 30.0), 30.0, gc.RX_POS[2]), [near],
                           [[30e3, 40e3, gc.RX_POS[2]]]])


@functools.lru_cache(maxsize=None)
def beam_reference():
    cfg, trials = _row_trials(BEAM_CASE)
    out = beam_ref.reference_rows(cfg, gc.SEED, trials, ITERS, beam_probes(), True, chunk=4)
    for a in out:
        a.setflags(write=False)
    return out


def test_beam_rows():
    """Case 4's system: per-trial beam rows within beam_ref.row_bounds, unchanged."""
    cfg, trials = _row_trials(BEAM_CASE)
    probes = beam_probes()
    assert probes.shape == (9, 3)
    d = np.linalg.norm(cfg.tx_pos[None] - probes[:, None], axis=2)
    assert abs(d[7, 0] - 3.0) < 1e-12 and d[7].max() / d[7].min() > 10 and 49e3 < d[8].min() < 51e3
    ref_counts, ref_rows, bounds = beam_reference()
    np.testing.assert_array_equal(ref_counts, gc.reference(BEAM_CASE)[:len(trials)])
    eng = engine_for(cfg, precision="f64")
    err, bits, beam, per, per_beam = eng.beam(gc.SEED, 0, len(trials), ITERS, probes, True, per_trial=True)
    eng.close()
    assert_counts_equal(per, ref_counts, "beam vs oracle")
    assert per_beam.shape == ref_rows.shape == (len(trials), 9, beam_ref.BEAM_FIXED)
    assert np.all(np.isfinite(per_beam))
    ratio = np.abs(per_beam - ref_rows) / bounds
    print(f"GEOMETRY_BEAM_RATIO case={gc.case_id(BEAM_CASE)} worst={ratio.max():.3e} per_probe="
          + ",".join(f"{v:.2e}" for v in ratio.max(axis=(0, 2))))
    assert ratio.max() <= 1.0, f"a beam row deviates {ratio.max():.3g} x its bound"
    np.testing.assert_allclose(beam, per_beam.sum(0), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- through Link
LINKS = {
    # array, n_ant of build_link, channel
    "planar_los": ("planar", (2, 4), "los"),
    "circular_two_path": ("circular", 8, "two_path"),
    "linear_rayleigh": ("linear", 8, "rayleigh"),
}
LINK_TRIALS = 24


@pytest.mark.parametrize("name", sorted(LINKS))
def test_link_on_the_geometry_vs_oracle(name):
    """The host mirror's own arrays, user and carriers reach the engine as the oracle sees them:
    Link.engine() on a PlanarRectangularArray, a CircularArray and a LinearArray at 100 MHz and
    120 kHz, F 512, S 256, user at (12, 7, 1.5) jittered over 4 m: per-trial counts EXACTLY those of
    the oracle given the link's positions (float64)."""
    from link_util import build_link
    array, n, chan = LINKS[name]
    F, S, M, ibo = 512, 256, 64, 2.0
    snr = float(rm.ebn0_to_snr(14.0, F, S, M))
    link, _ = build_link(n_ant=n, n_sc=S, n_fft=F, M=M, cp=16, ibo=ibo, chan=chan, array=array, center_freq=100e6,
                         carrier_spacing=120e3, rx_xyz=gc.RX_POS, rx_loc_var=gc.RX_LOC_VAR, precision="f64")
    link.set_snr(snr)
    pos = link.my_array.positions()
    assert pos.shape == (8, 3)
    cfg = sim.SimConfig(8, S, F, M, pa="softlim", ibo_db=ibo, snr_db=snr, channel=chan, tx_pos=pos, rx_pos=gc.RX_POS,
                        rx_loc_var=gc.RX_LOC_VAR, center_freq=100e6, carrier_spacing=120e3)
    ref = sim.run_trials(cfg, gc.SEED, np.arange(LINK_TRIALS), iters=ITERS, incl_clean=True)
    eng = link.engine()
    err, bits, per = eng.run(gc.SEED, 0, LINK_TRIALS, ITERS, True, per_trial=True)
    print(f"GEOMETRY_LINK {name} [{eng.describe()}] agreement={count_agreement(per, ref):.4f} "
          f"gpu={per.sum(0).tolist()} oracle={ref.sum(0).tolist()}")
    assert ref.sum(0).min() >= 20
    assert_counts_equal(per, ref, f"link {name}")
    np.testing.assert_array_equal(err, ref.sum(0))
