"""Soft mode of the fused trial kernel (mimo_engine_soft_points) on the GPU: the same counts as the
plain run and the oracle, and per trial and counter index the histogram of the bit reliabilities
equal to the oracle-built reference (tests/soft_ref.py) cell for cell.

The histograms can be compared exactly because, on these cases, no reliability lies within the
allowed error of a bin edge (``near_edge == 0``; the edge at 0 is the hard decision's) and none is
exactly 0 -- conditions on the inputs that every case asserts on the reference before it looks at
the device, with "every index's row sums to S log2 M" and "the cells below bin 128 sum to the
oracle's error count".
"""
import dataclasses
import functools

import numpy as np
import pytest

import soft_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import sim

pytestmark = pytest.mark.gpu

SEED = 7
N_TRIALS = 8
RHO_MAX = 16.0
NB = soft_ref.SOFT_BINS

# the smallest shapes that reach every variant: (config, iters, incl_clean, rho_max, seed)
CASES = {
    # generic band (a partial valid_mask), one wave, and the clean index
    "f256_generic": (dict(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                          channel="rayleigh"), (0, 1, 2), True, RHO_MAX, SEED),
    # the same system, iteration 1 run but not recorded: it must leave no cells
    "f256_skip": (dict(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                       channel="rayleigh"), (0, 2), True, RHO_MAX, SEED),
    # hb = 1: one bit per axis, only the top-bit rule
    "f128_qpsk": (dict(n_ant=4, n_sc=64, n_fft=128, constel_size=4, pa="softlim", ibo_db=0.0, snr_db=8.0,
                       channel="rayleigh"), (0, 1), False, RHO_MAX, SEED),
    # aligned, 4 slots
    "f512_16qam": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0,
                        channel="rayleigh"), (0, 1), False, RHO_MAX, SEED),
    # the CSI instance: its clean run combines with cc
    "f512_csi": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0,
                      channel="rayleigh", csi_eps=0.2), (0, 1), True, RHO_MAX, SEED),
    # closed-form channel
    "f512_los": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                      channel="los"), (0, 1), False, RHO_MAX, SEED),
    # wave-split FFT, T 256: the MCNC loop's detect
    "f2048_mcnc": (dict(n_ant=4, n_sc=1024, n_fft=2048, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                        channel="rayleigh", receiver="mcnc"), (0, 1, 2), False, RHO_MAX, SEED),
    # 8 slots, 16-point team
    "f4096_rapp": (dict(n_ant=2, n_sc=2048, n_fft=4096, constel_size=64, pa="rapp", p_hardness=3.0, ibo_db=3.0,
                        snr_db=25.0, channel="rayleigh"), (0, 1), False, RHO_MAX, SEED),
    # split FFT, T 512: the LDS is full
    "f8192": (dict(n_ant=2, n_sc=4096, n_fft=8192, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0,
                   channel="rayleigh"), (0, 1), False, RHO_MAX, SEED),
    # hb = 6; |lambda| reaches 64^2 / 4 = 1,024 at the outer levels, so rho_max 2,048 covers the range
    "f256_4096qam": (dict(n_ant=4, n_sc=128, n_fft=256, constel_size=4096, pa="none", ibo_db=3.0, snr_db=45.0,
                          channel="rayleigh"), (0,), False, 2048.0, SEED),
    # every counter index: n_idx 33, a row of 8,448 doubles
    "f128_all_idx": (dict(n_ant=4, n_sc=64, n_fft=128, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=14.0,
                          channel="rayleigh"), tuple(range(32)), True, RHO_MAX, SEED),
}


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS, rho_max=None):
    """(config, counts, rows [n, n_idx, 256], near-edge count, exact zeros) of a case."""
    kw, iters, clean, rmax, seed = CASES[name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    counts, rows, near, nz = soft_ref.reference(cfg, seed, np.arange(first, first + n), iters,
                                                rmax if rho_max is None else rho_max, clean)
    for a in (counts, rows):
        a.setflags(write=False)
    return cfg, counts, rows, near, nz


def assert_reference_conditions(name, cfg, counts, rows, near, nz):
    """The conditions on the inputs, on the reference alone."""
    assert near == 0, f"{name}: {near} reliabilities near a bin edge"
    assert nz == 0, f"{name}: {nz} reliabilities are exactly 0"
    n_rel = cfg.n_sc * int(np.log2(cfg.constel_size))
    assert np.all(rows.sum(axis=2) == n_rel), f"{name}: a row does not sum to S log2 M"
    np.testing.assert_array_equal(rows[:, :, :128].sum(axis=2), counts, err_msg=f"{name}: negatives vs counts")


@pytest.mark.parametrize("name", sorted(CASES))
def test_soft_rows_and_counts(name):
    kw, iters, clean, rho_max, seed = CASES[name]
    cfg, ref_counts, ref_rows, near, nz = reference(name)
    assert_reference_conditions(name, cfg, ref_counts, ref_rows, near, nz)
    n_idx = len(iters) + int(clean)
    eng = engine_for(cfg, precision="f64")
    err, bits, soft, per, per_soft = eng.soft(seed, 0, N_TRIALS, iters, rho_max, incl_clean=clean, per_trial=True)
    soft_ms = eng.kernel_ms
    assert soft_ms > 0  # mimo_engine_last_kernel_ms covers the mode's kernel
    e_run, b_run, per_run = eng.run(seed, 0, N_TRIALS, iters, incl_clean=clean, per_trial=True)
    print(name, eng.describe(), "counts", per.sum(0), "kernel ms", soft_ms)
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: soft vs run")
    assert_counts_equal(per, ref_counts, f"{name}: soft vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    # per-trial rows: the reference's, cell for cell
    assert per_soft.shape == ref_rows.shape == (N_TRIALS, n_idx, NB) and soft.shape == (n_idx, NB)
    np.testing.assert_array_equal(per_soft, ref_rows, err_msg=f"{name}: per-trial rows")
    # totals: the column sums, exactly
    np.testing.assert_array_equal(soft, per_soft.sum(axis=0))
    eng.close()


def test_unrecorded_iteration_leaves_no_cells():
    """iters (0, 2) against (0, 1, 2) of the same system: indices clean, 0 and 2 are the same rows."""
    _, _, rows_all, _, _ = reference("f256_generic")
    _, _, rows_skip, _, _ = reference("f256_skip")
    np.testing.assert_array_equal(rows_skip, rows_all[:, [0, 1, 3]])
    kw, iters, clean, rho_max, seed = CASES["f256_skip"]
    eng = engine_for(sim.SimConfig(**kw), precision="f64")
    _, _, soft_a, _, per_a = eng.soft(seed, 0, N_TRIALS, (0, 1, 2), rho_max, incl_clean=True, per_trial=True)
    _, _, soft_s, _, per_s = eng.soft(seed, 0, N_TRIALS, iters, rho_max, incl_clean=True, per_trial=True)
    eng.close()
    np.testing.assert_array_equal(per_s, per_a[:, [0, 1, 3]])
    np.testing.assert_array_equal(soft_s, soft_a[[0, 1, 3]])


def test_soft_points_rows_and_repeatability():
    """Case 1's system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, one call."""
    name = "f256_generic"
    _, iters, clean, rho_max, seed = CASES[name]
    ibos, n_trials, first = (0.0, 3.0, 6.0), (5, 3, 4), (0, 16, 40)
    refs = [reference(name, ibo, f, n) for ibo, f, n in zip(ibos, first, n_trials)]
    for r in refs:
        assert_reference_conditions(name, *r)
    eng = engine_for(refs[1][0], precision="f64")
    points = []
    for r in refs:
        e = engine_for(r[0], precision="f64")
        points.append(dict(e.point_kw))
        e.close()
    seeds = [seed] * 3
    err, bits, soft, per, per_soft = eng.soft_points(points, seeds, first, n_trials, iters, rho_max, clean, True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, clean, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "soft_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[1] for r in refs]), "soft_points vs oracle")
    np.testing.assert_array_equal(per_soft, np.concatenate([r[2] for r in refs]))
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(3):
        own = per_soft[off[i]:off[i + 1]]
        np.testing.assert_array_equal(soft[i], own.sum(axis=0))
        # every point's rows and totals are those of a single-point call, bit for bit
        _, _, s1, _, ps1 = eng.soft(seeds[i], first[i], n_trials[i], iters, rho_max, clean, True, point=points[i])
        np.testing.assert_array_equal(ps1, own)
        np.testing.assert_array_equal(s1, soft[i])
    # a second identical call: bit-identical totals and rows
    _, _, soft2, _, per_soft2 = eng.soft_points(points, seeds, first, n_trials, iters, rho_max, clean, True)
    np.testing.assert_array_equal(soft2, soft)
    np.testing.assert_array_equal(per_soft2, per_soft)
    eng.close()


def test_soft_totals_across_slices_and_launches(monkeypatch):
    """More trials than one reduction slice (4096), and a call split into several launches
    (MIMO_MAX_LAUNCH_TRIALS): the totals are the per-trial rows' sums, and rows, counts and totals
    do not depend on the splitting."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0)
    eng = engine_for(cfg, precision="f64")
    n = 4096 + 37
    err, _, soft, per, ps = eng.soft(SEED, 0, n, (0, 1), RHO_MAX, per_trial=True)
    np.testing.assert_array_equal(soft, ps.sum(axis=0))
    assert np.all(soft.sum(axis=1) == n * 128 * 6)
    np.testing.assert_array_equal(err, per.sum(0))
    np.testing.assert_array_equal(soft[:, :128].sum(axis=1), err)
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "1500")
    err3, _, soft3, per3, ps3 = eng.soft(SEED, 0, n, (0, 1), RHO_MAX, per_trial=True)
    np.testing.assert_array_equal(ps3, ps)
    np.testing.assert_array_equal(per3, per)
    np.testing.assert_array_equal(err3, err)
    np.testing.assert_array_equal(soft3, soft)
    monkeypatch.delenv("MIMO_MAX_LAUNCH_TRIALS")
    _, _, soft4, _, ps4 = eng.soft(SEED, 0, n, (0, 1), RHO_MAX, per_trial=True)
    np.testing.assert_array_equal(soft4, soft)
    np.testing.assert_array_equal(ps4, ps)
    eng.close()


def test_link_soft_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM, soft limiter at IBO 1
    link.set_snr(14.0)
    pp = link.point_params()
    nominal = 4.0 * 10 ** 1.4 / pp["avg_symbol_power"]
    assert link.nominal_llr_scale() == nominal
    st = link.soft(True, True, [0, 1, 2], [11, 22, 33], N_TRIALS)
    assert (st.n_idx, st.n_trials, st.constel_size, st.rho_max) == (4, N_TRIALS, 16, 32.0 / nominal)
    eng = link.engine()
    err, bits, soft, _, _ = eng.soft(_seed64([11, 22, 33]), 0, N_TRIALS, [0, 1, 2], 32.0 / nominal, incl_clean=True,
                                     point=link.point_params())
    np.testing.assert_array_equal(st.hist, soft)
    assert np.all(st.n_bits == N_TRIALS * 64 * 4) and np.all(bits == N_TRIALS * 64 * 4)
    # an explicit rho_max, and soft_points at two IBOs: point 0 is the call above
    st2 = link.soft(True, True, [0, 1, 2], [11, 22, 33], N_TRIALS, rho_max=2.0)  # narrower than the default 3.18
    assert st2.rho_max == 2.0 and np.all(st2.clamped() >= st.clamped())
    np.testing.assert_array_equal(st2.ber(), st.ber())
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.soft_points(True, True, [0, 1, 2], [[11, 22, 33], [5]], [p0, p1], N_TRIALS)
    np.testing.assert_array_equal(both[0].hist, st.hist)
    assert both[1].rho_max == st.rho_max


def test_soft_stats_of_a_case():
    """SoftStats.ber() x bits = the error counts, and 0 <= gmi(nominal) <= gmi() <= 1."""
    import _engine
    name = "f512_16qam"
    kw, iters, clean, rho_max, seed = CASES[name]
    cfg = sim.SimConfig(**kw)
    eng = engine_for(cfg, precision="f64")
    err, bits, soft, _, _ = eng.soft(seed, 0, N_TRIALS, iters, rho_max, incl_clean=clean)
    eng.close()
    st = _engine.SoftStats(soft, rho_max, cfg.constel_size, N_TRIALS)
    np.testing.assert_array_equal(st.n_bits, bits)
    # ber() bits = err: the cells below bin 128 are the errors, and ber() is their one division by N
    np.testing.assert_array_equal(st.hist[:, :128].sum(axis=1), err)
    np.testing.assert_array_equal(st.ber(), err / bits)
    pp = sim.point_params(cfg)
    nominal = st.nominal_scale(pp["es"] / pp["snr"])
    g_nom, g_max = st.gmi(nominal), st.gmi()
    print("SOFT_GMI", name, "ber", st.ber(), "gmi(nominal)", g_nom, "gmi()", g_max, "scale", st.best_scale(), nominal)
    assert np.all(0 <= g_nom) and np.all(g_nom <= g_max) and np.all(g_max <= 1)
    np.testing.assert_array_equal(st.rate(), 4 * g_max)
