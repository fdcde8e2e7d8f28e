"""The oracle's receiver-PA fields (SimConfig.cnc_pa / cnc_ibo_db / cnc_toi_coeff) on the CPU: at
their defaults the goldens are reproduced, set they change what the CNC receiver counts and nothing
else, and the mixed-point list of tests/point_mix.py can tell its points apart."""
import dataclasses

import numpy as np
import pytest

import measure_ref
import point_mix as pm
from conftest import link_fixture_names, load_golden, sim_config_from_fixture
from oracle import refmath as rm
from oracle import sim


GOLDENS = ("a8_cnc", "rapp")  # a soft-limiter and a Rapp link fixture, both under the CNC receiver


def _golden(name):
    g = load_golden(f"link_{name}.npz")
    return g, sim_config_from_fixture(g)


def _counts(cfg, g):
    n = int(g["n_trials"])
    return sim.run_trials(cfg, int(g["seed"]), np.arange(n), iters=g["iters"], incl_clean=bool(g["incl_clean"]))


@pytest.mark.parametrize("name", GOLDENS)
def test_receiver_fields_at_their_defaults_reproduce_the_goldens(name):
    assert name in link_fixture_names()
    g, cfg = _golden(name)
    assert (cfg.cnc_pa, cfg.cnc_ibo_db, cfg.cnc_toi_coeff) == (None, None, None) and cfg.receiver == "cnc"
    np.testing.assert_array_equal(_counts(cfg, g), g["counts"])
    # the fields spelled out as the array's: the same point, the same counts
    same = dataclasses.replace(cfg, cnc_pa=cfg.pa, cnc_ibo_db=cfg.ibo_db)
    for k, v in sim.point_params(cfg).items():
        if k != "const":
            assert sim.point_params(same)[k] == v, k
    np.testing.assert_array_equal(_counts(same, g), g["counts"])


@pytest.mark.parametrize("name", GOLDENS)
def test_a_set_receiver_pa_changes_the_cnc_counts_and_only_them(name):
    g, cfg = _golden(name)
    iters = [int(i) for i in g["iters"]]
    assert iters[0] == 0 and max(iters) >= 1 and bool(g["incl_clean"])
    first_it = 2  # the clean run and the standard receiver (iteration 0) do not see the receiver's PA
    for kw in (dict(cnc_pa="none"), dict(cnc_pa="toi", cnc_ibo_db=6.0), dict(cnc_ibo_db=cfg.ibo_db + 3.0),
               dict(cnc_pa="rapp" if cfg.pa == "softlim" else "softlim")):
        got = _counts(dataclasses.replace(cfg, **kw), g)
        np.testing.assert_array_equal(got[:, :first_it], g["counts"][:, :first_it])
        assert not np.array_equal(got[:, first_it:], g["counts"][:, first_it:]), kw
    # MCNC re-transmits through the array's PA: the fields are ignored
    mcnc = dataclasses.replace(cfg, receiver="mcnc")
    np.testing.assert_array_equal(_counts(dataclasses.replace(mcnc, cnc_pa="none", cnc_ibo_db=9.0, cnc_toi_coeff=0.3), g),
                                  _counts(mcnc, g))


def test_point_params_derive_the_receiver_fields_with_the_array_formulas():
    cfg = sim.SimConfig(8, 256, 512, 16, pa="rapp", ibo_db=1.0)
    base = sim.point_params(cfg)
    avg = base["avg_samp"]
    assert base["cnc_pa"] == "rapp" and base["cnc_sat"] == rm.sat_pow(1.0, avg) and base["cnc_coeff"] == 0.0
    pp = sim.point_params(dataclasses.replace(cfg, cnc_pa="softlim", cnc_ibo_db=2.5))
    assert pp["cnc_pa"] == "softlim" and pp["cnc_sat"] == rm.sat_pow(2.5, avg)
    assert pp["cnc_alpha"] == base["cnc_alpha"] == float(rm.calc_alpha(1.0))  # alpha stays the array's
    pp = sim.point_params(dataclasses.replace(cfg, cnc_pa="toi", cnc_ibo_db=6.0))
    assert pp["cnc_coeff"] == rm.toi_coeff(6.0, avg) and pp["cnc_sat"] == 0.0 and pp["cnc_alpha"] == base["cnc_alpha"]
    pp = sim.point_params(dataclasses.replace(cfg, cnc_pa="toi", cnc_toi_coeff=0.125, cnc_alpha=0.8))
    assert pp["cnc_coeff"] == 0.125 and pp["cnc_alpha"] == 0.8
    toi = sim.SimConfig(8, 256, 512, 16, pa="toi", ibo_db=6.0)
    assert sim.point_params(toi)["cnc_alpha"] == 1.0 and sim.point_params(toi)["cnc_pa"] == "toi"


def test_measure_reference_follows_the_receiver_pa():
    """tests/measure_ref.py hands its CNC loop the receiver's kind: the iteration columns of its rows
    move with cnc_pa, the signal columns and the standard receiver's do not."""
    cfg = pm.base_config("f256_generic", **pm.MIX[7][0])
    twin = pm.base_config("f256_generic", **pm.matched(7))
    c1, r1, _ = measure_ref.reference_rows(cfg, 107, np.arange(2), pm.ITERS, True)
    c0, r0, _ = measure_ref.reference_rows(twin, 107, np.arange(2), pm.ITERS, True)
    np.testing.assert_array_equal(c1, sim.run_trials(cfg, 107, np.arange(2), iters=pm.ITERS, incl_clean=True))
    np.testing.assert_array_equal(r1[:, :measure_ref.MEAS_FIXED + 2], r0[:, :measure_ref.MEAS_FIXED + 2])
    assert np.all(r1[:, measure_ref.MEAS_FIXED + 2:] != r0[:, measure_ref.MEAS_FIXED + 2:])


@pytest.mark.parametrize("shape", sorted(pm.SHAPES))
def test_the_mixed_points_can_be_told_apart(shape):
    """A condition on the inputs of the GPU test, not on the kernel: every point's trials count
    differently under the parameters of the point before and of the point after it, and every
    mismatch point differently from its twin whose receiver copies the array's PA."""
    assert pm.neighbours_differ(shape) == []
    assert pm.mismatch_differs(shape) == []
    if shape == "f512_aligned":
        assert pm.neighbours_differ(shape, "mcnc", pm.BASE) == []
        # pinned: 4 trials of seed 107, a Rapp array with a Rapp / a soft-limiter receiver; every trial differs
        assert pm.oracle_counts_matched(shape, 7).sum(0).tolist() == [1, 3, 69, 95]
        assert pm.oracle_counts(shape, 7).sum(0).tolist() == [1, 3, 106, 128]
        assert np.all(np.any(pm.oracle_counts(shape, 7) != pm.oracle_counts_matched(shape, 7), axis=1))
