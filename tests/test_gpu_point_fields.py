"""Every mimo_point field in launches that mix them (mimo_engine_run_points and its measure, spectrum
and beam siblings), on the GPU.

The kernels fetch a block's parameters from ``points[pi]``; the other multi-point tests vary IBO and
SNR only, over soft limiters.  Here one launch holds the list of tests/point_mix.py -- soft limiter,
Rapp at hardness 3 / 2.5 / 2 (the two integer kernels and the general one), the cubic model, no PA,
a fixed array gain, a CNC receiver whose PA copy differs from the array's in kind, in saturation
power and in cubic coefficient, and a point without trials -- with neighbours that differ in kind,
own seeds and own first trials.  Counts are compared exactly (the oracle sees the device's Philox
draws); rows of the measure, spectrum and beam modes within the bounds of their reference modules.
That the list can tell its points apart is asserted on the oracle alone
(tests/test_oracle_receiver_pa.py and again here, from the cached counts).

Measured totals and worst row-to-bound ratios: profiles/r12/point_fields/README.md.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import beam_ref
import measure_ref
import point_mix as pm
import spectrum_ref
from gpu_util import PRECISIONS, assert_counts_equal, engine_for
from oracle import refmath as rm
from oracle import sim
from utilities import circle_probes

pytestmark = pytest.mark.gpu

ITERS, CLEAN = pm.ITERS, pm.CLEAN
N_IDX = len(ITERS) + int(CLEAN)
SHAPE_NAMES = sorted(pm.SHAPES)


def bits_per_trial(cfg):
    return cfg.n_sc * rm.bits_per_symbol(cfg.constel_size)


def mixed_launch(eng, shape, which=None, receiver="cnc"):
    """run_points over the list -> (err, bits, [per-trial counts of each point])."""
    cfgs = pm.configs(shape, receiver, which)
    seeds, firsts, ns = pm.launch_args(which)
    err, bits, per = eng.run_points([pm.point_of(c) for c in cfgs], seeds, firsts, ns, ITERS, CLEAN, per_trial=True)
    assert per.shape == (sum(ns), N_IDX)
    return err, bits, np.split(per, np.cumsum(ns)[:-1])


def first_engine(shape, prec, receiver="cnc"):
    """An engine of the shape; its set_point is point 0, which no multi-point call reads."""
    return engine_for(pm.configs(shape, receiver, [0])[0], precision=prec)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_mixed_launch_equals_the_oracle(shape, prec):
    assert pm.neighbours_differ(shape) == [] and pm.mismatch_differs(shape) == []  # the list has teeth
    eng = first_engine(shape, prec)
    err, bits, got = mixed_launch(eng, shape)
    cfgs = pm.configs(shape)
    print(shape, prec, eng.describe())
    for i, cfg in enumerate(cfgs):
        ref = pm.oracle_counts(shape, i)
        print(f"POINT_FIELDS shape={shape} prec={prec} point={i} oracle={ref.sum(0).tolist()} "
              f"gpu={got[i].sum(0).tolist()}")
    for i, cfg in enumerate(cfgs):
        ref = pm.oracle_counts(shape, i)
        assert_counts_equal(got[i], ref, f"{shape} {prec} point {i}")
        np.testing.assert_array_equal(err[i], ref.sum(0))
        assert np.all(bits[i] == pm.MIX[i][1] * bits_per_trial(cfg))
    z = pm.ZERO_TRIAL_POINT
    assert got[z].shape == (0, N_IDX) and not err[z].any() and not bits[z].any()
    eng.close()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_mixed_launch_equals_single_point_launches(shape, prec):
    """The fetch property without any rounding question: on one engine, every point's rows in the
    mixed launch are those of a launch of that point alone (n_points = 1: no search, point 0), bit
    for bit -- and of mimo_engine_run after set_point."""
    eng = first_engine(shape, prec)
    err, bits, got = mixed_launch(eng, shape)
    for i, cfg in enumerate(pm.configs(shape)):
        e1, b1, g1 = mixed_launch(eng, shape, [i])
        np.testing.assert_array_equal(g1[0], got[i], err_msg=f"{shape} {prec} point {i}")
        np.testing.assert_array_equal(e1[0], err[i])
        np.testing.assert_array_equal(b1[0], bits[i])
        _, n, seed, first = pm.MIX[i]
        eng.set_point(**pm.point_of(cfg))
        e2, b2, g2 = eng.run(seed, first, n, ITERS, CLEAN, per_trial=True)
        np.testing.assert_array_equal(g2, got[i], err_msg=f"{shape} {prec} point {i} (run)")
        np.testing.assert_array_equal(e2, err[i])
    # the list reversed: every point at another block range, after other neighbours
    rev = list(range(len(pm.MIX)))[::-1]
    e3, b3, g3 = mixed_launch(eng, shape, rev)
    for k, i in enumerate(rev):
        np.testing.assert_array_equal(g3[k], got[i], err_msg=f"{shape} {prec} point {i} (reversed)")
        np.testing.assert_array_equal(e3[k], err[i])
    eng.close()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_mixed_launch_does_not_depend_on_the_launch_splitting(shape, prec, monkeypatch):
    """MIMO_MAX_LAUNCH_TRIALS = 3: launches begin and end inside points (4 and 5 trials) and hold
    the end of one point with the start of the next.  Rows and totals are identical."""
    eng = first_engine(shape, prec)
    err, bits, got = mixed_launch(eng, shape)
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "3")
    err3, bits3, got3 = mixed_launch(eng, shape)
    for i in range(len(pm.MIX)):
        np.testing.assert_array_equal(got3[i], got[i], err_msg=f"{shape} {prec} point {i}")
    np.testing.assert_array_equal(err3, err)
    np.testing.assert_array_equal(bits3, bits)
    eng.close()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_receiver_pa_mismatch_points_alone(shape, prec):
    """A CNC receiver whose PA copy is not the array's -- another kind, another saturation power,
    another cubic coefficient -- each as the engine's only point: exact against the oracle, whose
    counts with a matching receiver differ (a swap of sat_cnc / sat_tx or toi_cnc / toi_tx in the
    receiver's PA call, or cnc_pa_kind read as pa_kind, would give those)."""
    assert pm.mismatch_differs(shape) == []
    for i in pm.MISMATCH:
        cfg = pm.configs(shape, which=[i])[0]
        _, n, seed, first = pm.MIX[i]
        eng = engine_for(cfg, precision=prec)
        err, bits, per = eng.run(seed, first, n, ITERS, CLEAN, per_trial=True)
        twin = pm.oracle_counts_matched(shape, i)
        print(f"POINT_FIELDS_MISMATCH shape={shape} prec={prec} point={i} oracle={pm.oracle_counts(shape, i).sum(0).tolist()} "
              f"gpu={per.sum(0).tolist()} matched_receiver={twin.sum(0).tolist()}")
        assert_counts_equal(per, pm.oracle_counts(shape, i), f"{shape} {prec} point {i}")
        np.testing.assert_array_equal(err, pm.oracle_counts(shape, i).sum(0))
        assert not np.array_equal(per, twin)
        eng.close()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_an_infinite_saturation_power_is_no_pa(prec):
    """sat_pow = cnc_sat_pow = +inf, which the point validation accepts: a soft limiter and a Rapp
    model (integer and general hardness) that never saturate count, trial for trial, what the same
    trials count without a PA -- in one launch, next to that point."""
    shape, i_none = "f512_aligned", 4
    cfg = pm.configs(shape, which=[i_none])[0]
    assert cfg.pa == "none"
    _, n, seed, first = pm.MIX[i_none]
    none = pm.point_of(cfg)
    inf = float("inf")
    pts = [dict(none, pa_kind="softlim", cnc_pa_kind="softlim", sat_pow=inf, cnc_sat_pow=inf),
           none,
           dict(none, pa_kind="rapp", cnc_pa_kind="rapp", p_hardness=3.0, sat_pow=inf, cnc_sat_pow=inf),
           dict(none, pa_kind="rapp", cnc_pa_kind="softlim", p_hardness=2.5, sat_pow=inf, cnc_sat_pow=inf)]
    eng = first_engine(shape, prec)
    err, bits, per = eng.run_points(pts, [seed] * 4, [first] * 4, [n] * 4, ITERS, CLEAN, per_trial=True)
    got = np.split(per, 4)
    assert_counts_equal(got[1], pm.oracle_counts(shape, i_none), f"no PA {prec}")
    for k in (0, 2, 3):
        assert_counts_equal(got[k], got[1], f"{pts[k]['pa_kind']} at sat_pow = inf vs no PA, {prec}")
    eng.close()


# ---------------------------------------------------------------- CSI error per point
CSI_EPS = (0.0, 0.1, 0.3)
CSI_SEEDS, CSI_FIRST, CSI_N = (120, 121, 122), (0, 6, 50), (3, 4, 3)


@functools.lru_cache(maxsize=None)
def csi_reference(k, eps):
    cfg = pm.base_config("f512_aligned", pa="softlim", ibo_db=1.0, csi_eps=eps)
    ref = sim.run_trials(cfg, CSI_SEEDS[k], np.arange(CSI_FIRST[k], CSI_FIRST[k] + CSI_N[k]), iters=ITERS,
                         incl_clean=CLEAN)
    ref.setflags(write=False)
    return cfg, ref


@pytest.mark.parametrize("prec", PRECISIONS)
def test_csi_eps_differs_between_the_points_of_one_launch(prec):
    refs = [csi_reference(k, eps) for k, eps in enumerate(CSI_EPS)]
    # teeth, on the oracle: each point's trials under a neighbour's epsilon count differently
    for k in range(3):
        for j in (k - 1, k + 1):
            if 0 <= j < 3:
                assert not np.array_equal(csi_reference(k, CSI_EPS[j])[1], refs[k][1]), (k, j)
    eng = engine_for(refs[1][0], precision=prec)
    err, bits, per = eng.run_points([pm.point_of(r[0]) for r in refs], CSI_SEEDS, CSI_FIRST, CSI_N, ITERS, CLEAN,
                                    per_trial=True)
    got = np.split(per, np.cumsum(CSI_N)[:-1])
    for k, (cfg, ref) in enumerate(refs):
        print(f"POINT_FIELDS_CSI prec={prec} eps={CSI_EPS[k]} oracle={ref.sum(0).tolist()} gpu={got[k].sum(0).tolist()}")
    for k, (cfg, ref) in enumerate(refs):
        assert_counts_equal(got[k], ref, f"csi_eps {CSI_EPS[k]} {prec}")
        np.testing.assert_array_equal(err[k], ref.sum(0))
    # csi_eps = 0.0 is the error model with no error: the counts of the same trials on a perfect-CSI
    # engine (another kernel instance), and the oracle agrees
    perfect = dataclasses.replace(refs[0][0], csi_eps=None)
    ref_p = sim.run_trials(perfect, CSI_SEEDS[0], np.arange(CSI_FIRST[0], CSI_FIRST[0] + CSI_N[0]), iters=ITERS,
                           incl_clean=CLEAN)
    np.testing.assert_array_equal(ref_p, refs[0][1])
    eng_p = engine_for(perfect, precision=prec)
    _, _, per_p = eng_p.run(CSI_SEEDS[0], CSI_FIRST[0], CSI_N[0], ITERS, CLEAN, per_trial=True)
    assert "csi=0" in eng_p.describe() and "csi=1" in eng.describe()
    assert_counts_equal(per_p, got[0], f"perfect-CSI engine vs csi_eps = 0.0 {prec}")
    eng.close()
    eng_p.close()


# ---------------------------------------------------------------- MCNC: the array's fields only
@pytest.mark.parametrize("prec", PRECISIONS)
def test_mcnc_mixed_launch_and_ignored_receiver_fields(prec):
    shape = "f512_aligned"
    assert pm.neighbours_differ(shape, "mcnc", pm.BASE) == []
    eng = first_engine(shape, prec, "mcnc")
    err, bits, got = mixed_launch(eng, shape, pm.BASE, "mcnc")
    for i in pm.BASE:
        ref = pm.oracle_counts(shape, i, None, "mcnc")
        print(f"POINT_FIELDS_MCNC prec={prec} point={i} oracle={ref.sum(0).tolist()} gpu={got[i].sum(0).tolist()}")
    for i in pm.BASE:
        ref = pm.oracle_counts(shape, i, None, "mcnc")
        assert_counts_equal(got[i], ref, f"mcnc {prec} point {i}")
        np.testing.assert_array_equal(err[i], ref.sum(0))
    # valid but different cnc_* fields, another set per point: MCNC reads none of them
    other = [dict(cnc_pa_kind="toi", cnc_sat_pow=0.0, cnc_toi_coeff=0.3, cnc_alpha=0.5),
             dict(cnc_pa_kind="softlim", cnc_sat_pow=1e-3, cnc_toi_coeff=0.0, cnc_alpha=-2.0),
             dict(cnc_pa_kind="none", cnc_sat_pow=0.0, cnc_toi_coeff=7.0, cnc_alpha=1e6),
             dict(cnc_pa_kind="rapp", cnc_sat_pow=5.0, cnc_toi_coeff=0.0, cnc_alpha=0.1)]
    pts = [dict(pm.point_of(c), **other[i % len(other)]) for i, c in enumerate(pm.configs(shape, "mcnc", pm.BASE))]
    seeds, firsts, ns = pm.launch_args(pm.BASE)
    err2, bits2, per2 = eng.run_points(pts, seeds, firsts, ns, ITERS, CLEAN, per_trial=True)
    np.testing.assert_array_equal(per2, np.concatenate(got))
    np.testing.assert_array_equal(err2, err)
    np.testing.assert_array_equal(bits2, bits)
    eng.close()


# ---------------------------------------------------------------- measure, spectrum and beam modes
MODE_SHAPE = "f256_generic"
MODE_POINTS = list(range(8))  # points 0-7: every array PA, the fixed gain, the kind mismatch


def mode_probes():
    """9 probes on the half circle through the default user, at its height."""
    rx = pm.base_config(MODE_SHAPE).rx_pos
    return circle_probes(np.linspace(0.0, 180.0, 9), math.hypot(rx[0], rx[1]), rx[2])


@functools.lru_cache(maxsize=None)
def mode_reference(mode):
    """Per point (counts, rows, bound inputs) of the mode's reference module."""
    out = []
    for i in MODE_POINTS:
        cfg = pm.configs(MODE_SHAPE, which=[i])[0]
        _, n, seed, first = pm.MIX[i]
        trials = np.arange(first, first + n)
        if mode == "measure":
            r = measure_ref.reference_rows(cfg, seed, trials, ITERS, CLEAN)
        elif mode == "spectrum":
            r = spectrum_ref.reference_rows(cfg, seed, trials, ITERS, CLEAN)
        else:
            r = beam_ref.reference_rows(cfg, seed, trials, ITERS, mode_probes(), CLEAN)
        for a in r:
            a.setflags(write=False)
        out.append(r)
    return out


def mode_call(eng, mode, which):
    pts = [pm.point_of(c) for c in pm.configs(MODE_SHAPE, which=which)]
    seeds, firsts, ns = pm.launch_args(which)
    if mode == "measure":
        return eng.measure_points(pts, seeds, firsts, ns, ITERS, CLEAN, per_trial=True)
    if mode == "spectrum":
        return eng.spectrum_points(pts, seeds, firsts, ns, ITERS, CLEAN, per_trial=True)
    return eng.beam_points(pts, seeds, firsts, ns, ITERS, mode_probes(), CLEAN, per_trial=True)


@pytest.mark.parametrize("mode", ["measure", "spectrum", "beam"])
def test_mode_points_over_mixed_fields(mode):
    refs = mode_reference(mode)
    eng = first_engine(MODE_SHAPE, "f64")
    err, bits, tot, per, rows = mode_call(eng, mode, MODE_POINTS)
    e_run, b_run, got_run = mixed_launch(eng, MODE_SHAPE, MODE_POINTS)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, np.concatenate(got_run), f"{mode}_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[0] for r in refs]), f"{mode}_points vs oracle")
    for k, i in enumerate(MODE_POINTS):
        np.testing.assert_array_equal(refs[k][0], pm.oracle_counts(MODE_SHAPE, i))
    ref_rows = np.concatenate([r[1] for r in refs])
    assert rows.shape == ref_rows.shape and np.all(np.isfinite(rows))
    if mode == "measure":
        bound = measure_ref.row_bounds(ref_rows, np.concatenate([r[2] for r in refs]))
    elif mode == "spectrum":
        bound = spectrum_ref.row_bounds(ref_rows)
    else:
        bound = np.concatenate([r[2] for r in refs])
    ratio = np.abs(rows - ref_rows) / bound
    ns = pm.launch_args(MODE_POINTS)[2]
    off = np.concatenate(([0], np.cumsum(ns)))
    print(f"{mode.upper()}_RATIO case=point_fields worst={float(ratio.max()):.3e} per_point="
          + ",".join(f"{float(ratio[off[k]:off[k + 1]].max()):.2e}" for k in range(len(ns))))
    assert float(ratio.max()) <= 1.0, f"{mode}: per-trial row deviates {float(ratio.max()):.3g} x its bound"
    # every point's rows are those of a single-point call, bit for bit
    for k, i in enumerate(MODE_POINTS):
        _, _, _, per1, rows1 = mode_call(eng, mode, [i])
        np.testing.assert_array_equal(rows1, rows[off[k]:off[k + 1]], err_msg=f"{mode} point {i}")
        np.testing.assert_array_equal(per1, per[off[k]:off[k + 1]])
    eng.close()


# ---------------------------------------------------------------- large constellations
LARGE = {256: 24.0, 1024: 32.0, 4096: 40.0}  # M -> Eb/N0 [dB]
LARGE_SEED, LARGE_TRIALS = 7, 6


@functools.lru_cache(maxsize=None)
def large_reference(m):
    a, s, f = 4, 128, 256
    cfg = sim.SimConfig(a, s, f, m, pa="softlim", ibo_db=6.0, snr_db=float(rm.ebn0_to_snr(LARGE[m], s, s, m)))
    ref = sim.run_trials(cfg, LARGE_SEED, np.arange(LARGE_TRIALS), iters=ITERS, incl_clean=CLEAN)
    ref.setflags(write=False)
    return cfg, ref


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("m", sorted(LARGE))
def test_large_constellations_in_the_trial_kernel(m, prec):
    """256-, 1024- and 4096-QAM (4- to 6-bit axes, up to 12-bit Philox labels) through the array, a
    soft limiter and the CNC loop: exact against the oracle, with errors in every iteration column."""
    cfg, ref = large_reference(m)
    assert np.all(ref.sum(0)[1:] > 0)
    eng = engine_for(cfg, precision=prec)
    err, bits, per = eng.run(LARGE_SEED, 0, LARGE_TRIALS, ITERS, CLEAN, per_trial=True)
    print(f"POINT_FIELDS_LARGE M={m} prec={prec} oracle={ref.sum(0).tolist()} gpu={per.sum(0).tolist()}")
    assert_counts_equal(per, ref, f"{m}-QAM {prec}")
    np.testing.assert_array_equal(err, ref.sum(0))
    assert np.all(bits == LARGE_TRIALS * bits_per_trial(cfg))
    eng.close()
