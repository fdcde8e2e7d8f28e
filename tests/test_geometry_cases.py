"""CPU: pins the off-default case table of tests/geometry_cases.py and the array placements.

The conditions are on the inputs of tests/test_gpu_geometry.py, from the oracle alone: a case
that misses one is changed (seed, Eb/N0, trials), not the condition.  Measured figures per case:
profiles/r13/geometry/README.md.
"""
import numpy as np
import pytest

import geometry_cases as gc
from oracle import refmath as rm

C0 = 299792458.0


@pytest.mark.parametrize("num", gc.CASE_NUMBERS, ids=gc.case_id)
def test_counters_are_neither_empty_nor_saturated(num):
    """Every counter's total is at least 20 errors and at most 25 % of its bits: an empty or a
    saturated counter shows nothing."""
    cfg, trials = gc.case_config(num)
    ref = gc.reference(num)
    assert ref.shape == (len(trials), 1 + len(gc.ITERS)) and np.all(np.isfinite(ref)) and np.all(ref >= 0)
    bits = len(trials) * cfg.n_sc * int(np.log2(cfg.constel_size))
    tot = ref.sum(0)
    print("GEOMETRY_TOTALS", gc.case_id(num), tot.tolist(), "of", bits)
    assert np.all(tot >= 20), tot
    assert np.all(tot <= 0.25 * bits), (tot, bits)


@pytest.mark.parametrize("num", gc.CASE_NUMBERS, ids=gc.case_id)
def test_antennas_are_unequal_and_the_band_is_wide(num):
    """The mean antenna powers spread by a factor of 4 at least (the default geometry: 1.012),
    and the band leaves [0.93, 1.07] fc on both sides (the default: 1 +- 0.005), so fc / f_k
    exceeds 1.07 too."""
    cfg, _ = gc.case_config(num)
    spread = gc.antenna_power_spread(cfg)
    r = gc.band_ratio(cfg)
    print("GEOMETRY_INPUTS", gc.case_id(num), f"spread {spread:.2f} f/fc [{r.min():.4f}, {r.max():.4f}] "
          f"fc/f [{(1 / r).min():.4f}, {(1 / r).max():.4f}]")
    assert spread >= 4.0, spread
    assert r.min() < 0.93 and r.max() > 1.07, (r.min(), r.max())
    assert (1 / r).max() > 1.07
    assert np.all(rm.fftfreq_carriers(cfg.n_fft, cfg.carrier_spacing, cfg.center_freq) > 0)
    assert cfg.rx_pos[0] != cfg.rx_pos[1]  # or the y jitter's centre could not be told apart


@pytest.mark.parametrize("num", gc.CASE_NUMBERS, ids=gc.case_id)
def test_every_mutant_moves_a_quarter_of_the_entries(num):
    """Each mutant of the case's channel changes more than 25 % of the (trial, counter) entries:
    five times what the float32 criterion of tests/test_gpu_geometry.py forgives (5 %), so a kernel
    with that slip fails in both precisions."""
    cfg, _ = gc.case_config(num)
    ref = gc.reference(num)
    names = gc.mutants_for(cfg.channel)
    assert len(names) >= 3
    for name in names:
        changed = gc.mutant_counts(num, name) != ref
        print("GEOMETRY_MUTANT", gc.case_id(num), name, int(changed.sum()), "of", changed.size)
        assert changed.mean() > 0.25, (name, int(changed.sum()), changed.size)
    # ... and leaves the oracle as it found it
    np.testing.assert_array_equal(gc.run_oracle(*gc.case_config(num)), ref)


def test_the_default_geometry_hides_the_y_jitter_mutant():
    """What the table is for: with the user on x = y the y-jitter mutant is the oracle itself."""
    default = lambda n_ant, n_fft: {}  # noqa: E731
    for num in (2, 7):
        cfg, trials = gc.case_config(num, default)
        np.testing.assert_array_equal(gc.mutant_counts(num, "y_jittered_around_rx_y", default),
                                      gc.run_oracle(cfg, trials))


def test_sparse_positions():
    p = gc.sparse_positions(8)
    assert p.shape == (8, 3)
    np.testing.assert_array_equal(p[:, 1], [0, 3, 0, 3, 0, 3, 0, 3])
    np.testing.assert_allclose(p[[0, -1]], [[-20, 0, 5], [20, 3, 15]])
    np.testing.assert_array_equal(gc.sparse_positions(1), [[3.0, 0.0, 9.0]])
    assert np.ptp(np.diff(p[:, 0])) < 1e-12 and np.ptp(np.diff(p[:, 2])) < 1e-12


# ---------------------------------------------------------------- array placements
def _array(kind, n, fc=int(100e6)):
    from link_util import build_link
    link, _ = build_link(n_ant=n, array=kind, center_freq=fc, carrier_spacing=120e3, n_sc=64, n_fft=128)
    return link.my_array.positions(), C0 / fc


def test_linear_array_positions():
    """x = linspace(-(n - 1) s lambda / 2, +(n - 1) s lambda / 2), y = 0, z = cord_z: n elements
    in ascending x, centred on x = 0."""
    pos, lam = _array("linear", 8)
    assert pos.shape == (8, 3)
    np.testing.assert_allclose(pos[:, 0], (np.arange(8) - 3.5) * 0.5 * lam, rtol=1e-14, atol=1e-14)
    np.testing.assert_array_equal(pos[:, 1], 0.0)
    np.testing.assert_array_equal(pos[:, 2], 15.0)
    assert abs(pos[:, 0].sum()) < 1e-12 and np.all(np.diff(pos[:, 0]) > 0)
    np.testing.assert_allclose(pos, rm.ula_positions(8, 100e6, 0.5, 15.0), rtol=1e-14, atol=1e-14)


def test_circular_array_positions():
    """Element i of n at the angle pi i / n on the semicircle of radius lambda (n - 1) / (2 pi)
    around the origin, at height cord_z: counter-clockwise from (R, 0), the point at pi left out."""
    n = 8
    pos, lam = _array("circular", n)
    assert pos.shape == (n, 3)
    radius = lam * (n - 1) / (2 * np.pi)
    th = np.pi * np.arange(n) / n
    np.testing.assert_allclose(pos[:, 0], radius * np.cos(th), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(pos[:, 1], radius * np.sin(th), rtol=1e-14, atol=1e-14)
    np.testing.assert_array_equal(pos[:, 2], 15.0)
    np.testing.assert_allclose(np.hypot(pos[:, 0], pos[:, 1]), radius, rtol=1e-14)  # centred on the origin
    np.testing.assert_array_equal(pos[0, :2], [radius, 0.0])
    assert np.all(np.diff(np.arctan2(pos[:, 1], pos[:, 0])) > 0) and np.all(pos[:, 1] >= 0)
    # neighbours sit about half a wavelength apart (the arc lambda (n - 1) / (2 n))
    np.testing.assert_allclose(np.linalg.norm(np.diff(pos, axis=0), axis=1), 2 * radius * np.sin(np.pi / (2 * n)))


def test_planar_rectangular_array_positions():
    """2 per row x 4 per column on the x-z plane: the 4 column values run along x (outer, ascending),
    the 2 row values along z (inner, ascending), half a wavelength apart, centred on x = 0 and z = cord_z."""
    pos, lam = _array("planar", (2, 4))
    assert pos.shape == (8, 3)
    xs = (np.arange(4) - 1.5) * 0.5 * lam
    zs = 15.0 + (np.arange(2) - 0.5) * 0.5 * lam
    want = np.array([[x, 0.0, z] for x in xs for z in zs])
    np.testing.assert_allclose(pos, want, rtol=1e-14, atol=1e-14)
    np.testing.assert_array_equal(pos[:, 1], 0.0)
    assert abs(pos[:, 0].mean()) < 1e-12 and abs(pos[:, 2].mean() - 15.0) < 1e-12
    assert len({tuple(p) for p in pos.round(9)}) == 8


def test_build_link_defaults_are_the_reference_system():
    """The new keywords of link_util.build_link default to the system every earlier test built."""
    from link_util import build_link
    link, _ = build_link()
    rx = link.my_standard_rx
    assert (rx.cord_x, rx.cord_y, rx.cord_z, rx.center_freq, rx.carrier_spacing) == (212.0, 212.0, 1.5, 3500000000, 15000)
    assert type(rx.center_freq) is int and link.rx_loc_var == 10.0
    np.testing.assert_array_equal(link.my_array.positions(), rm.ula_positions(8, 3.5e9, 0.5, 15.0))
    assert type(link.my_array).__name__ == "LinearArray"
