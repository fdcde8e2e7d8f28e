"""Counts parity of the float64 wave-split instances where csrc/tuning.h's alpha-wave and draw-series
switches act (MIMO_ALPHA_WAVE, MIMO_P1_LN_DEG, MIMO_BM_LN_DEG, MIMO_BM_SIN_DEG): perfect-CSI
Rayleigh, soft limiter, against oracle/sim.py, per trial and exactly.

Shapes (A, S, F), the smallest that run the changed code (F 1024 is the smallest wave-split size:
T = 128, two waves, one region of vk partials; tests/test_gpu_pass1_sums.py):
  (1, 512, 1024)   a single antenna on a two-wave team: the fixed alpha wave and the one other;
  (3, 512, 1024)   A no multiple of W, 16 trials each;
  (5, 1024, 2048)  the bench instance (T = 256, four waves, three regions), 8 trials.
CNC iterations 0, 1, 2 and the clean column.  One MCNC case at the bench shape: its later passes
run the antenna loop without alpha.  One run_points launch of two IBO points: alpha's polynomial
differs per team.  One measure call at the bench shape within tests/measure_ref.py's bounds:
alpha's last bits move with the order of its sum, so the rows are held to those bounds and not
compared bit for bit.  These are the smallest shapes that reach the changed code, all of them aligned
Rayleigh: the other float64 instances of the two sizes, which carry the same series cuts and alpha
wave -- generic bands, LoS, two-path and table channels, CSI, every row mode -- run in
tests/test_gpu_wave_split_instances.py (the matrix of tests/wave_split_cases.py, on the geometry of
SHAPES["F1024"]).

One case per switch at its other value (a switch never changes counts): a variant library built by
    make -C csrc variant VOUT=../../abl/lib_<SWITCH>_<value>.so VFLAGS=-D<SWITCH>=<value>
gives the default library's counts on 256 trials of the bench shape; skipped where that library
was not built."""
import functools
import os
import re

import numpy as np
import pytest

import measure_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import sim
from test_gpu_pass1_sums import REPO, TUNING, _engine_from, _point_of

pytestmark = pytest.mark.gpu

SHAPES = {"A1": (1, 512, 1024, 16, 16), "F1024": (3, 512, 1024, 16, 16), "F2048": (5, 1024, 2048, 64, 8)}  # A, S, F, M, trials
ITERS = [0, 1, 2]
SEED = 4243
IBO_B = 1.5
MEAS_TRIALS = 4
# the two values of every switch (tuning.h)
VALUES = {"MIMO_ALPHA_WAVE": (0, -1), "MIMO_P1_LN_DEG": (4, 6), "MIMO_BM_LN_DEG": (5, 6), "MIMO_BM_SIN_DEG": (5, 7)}


def _cfg(shape, ibo=3.0, receiver="cnc"):
    a, s, f, m, _ = SHAPES[shape]
    return sim.SimConfig(a, s, f, m, pa="softlim", ibo_db=ibo, snr_db=16.0, receiver=receiver)


@functools.lru_cache(maxsize=None)
def _oracle(shape, ibo, seed, first, receiver="cnc", clean=True):
    n = SHAPES[shape][4]
    ref = sim.run_trials(_cfg(shape, ibo, receiver), seed, np.arange(first, first + n), iters=ITERS, incl_clean=clean)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("shape", list(SHAPES))
def test_counts_equal_oracle(shape):
    eng = engine_for(_cfg(shape), precision="f64")
    desc = eng.describe()
    assert "f64" in desc and "aligned" in desc, desc
    _, _, per = eng.run(SEED, 0, SHAPES[shape][4], ITERS, True, per_trial=True)
    ref = _oracle(shape, 3.0, SEED, 0)
    print(f"WAVE_BALANCE|{shape}|{desc}|gpu={per.sum(0).tolist()}|oracle={ref.sum(0).tolist()}")
    assert ref.sum() > 0
    assert_counts_equal(per, ref, shape)


def test_mcnc_counts_equal_oracle():
    shape = "F2048"
    eng = engine_for(_cfg(shape, receiver="mcnc"), precision="f64")
    _, _, per = eng.run(SEED, 0, SHAPES[shape][4], ITERS, False, per_trial=True)
    ref = _oracle(shape, 3.0, SEED, 0, "mcnc", False)
    print(f"WAVE_BALANCE|mcnc|{eng.describe()}|gpu={per.sum(0).tolist()}|oracle={ref.sum(0).tolist()}")
    assert ref.sum() > 0
    assert_counts_equal(per, ref, "mcnc")


def test_two_ibo_points_in_one_launch():
    shape = "F2048"
    n = SHAPES[shape][4]
    eng = engine_for(_cfg(shape), precision="f64")
    pts = [_point_of(_cfg(shape, 3.0)), _point_of(_cfg(shape, IBO_B))]
    err, _, per = eng.run_points(pts, [SEED, SEED + 1], [0, 5], [n, n], ITERS, True, per_trial=True)
    assert_counts_equal(per[:n], _oracle(shape, 3.0, SEED, 0), f"{shape} IBO 3")
    assert_counts_equal(per[n:], _oracle(shape, IBO_B, SEED + 1, 5), f"{shape} IBO {IBO_B}")
    np.testing.assert_array_equal(err[0], per[:n].sum(0))
    np.testing.assert_array_equal(err[1], per[n:].sum(0))


def test_measure_rows_within_bounds():
    cfg = _cfg("F2048")
    iters = (0, 1)
    ref_counts, ref_rows, ez = measure_ref.reference_rows(cfg, SEED, np.arange(MEAS_TRIALS), iters, False)
    eng = engine_for(cfg, precision="f64")
    _, _, meas, per, per_meas = eng.measure(SEED, 0, MEAS_TRIALS, iters, False, per_trial=True)
    assert_counts_equal(per, ref_counts, "measure vs oracle")
    assert per_meas.shape == ref_rows.shape and np.all(np.isfinite(per_meas))
    ratio = np.abs(per_meas - ref_rows) / measure_ref.row_bounds(ref_rows, ez)
    print("WAVE_BALANCE|measure|worst ratio to bound per column " + ",".join(f"{v:.2e}" for v in ratio.max(axis=0)))
    assert ratio.max() <= 1.0
    np.testing.assert_allclose(meas, per_meas.sum(0), rtol=1e-12, atol=0)


def _default_of(switch):
    with open(TUNING) as f:
        return int(re.search(r"#define %s (-?\d+)" % switch, f.read()).group(1))


@pytest.mark.parametrize("switch", list(VALUES))
def test_switch_keeps_counts(switch):
    a, b = VALUES[switch]
    default = _default_of(switch)
    assert default in (a, b)
    other = b if default == a else a
    path = os.path.join(REPO, "abl", f"lib_{switch}_{other}.so")
    if not os.path.exists(path):
        pytest.skip(f"variant library {os.path.relpath(path, REPO)} not built (make -C csrc variant)")
    cfg = _cfg("F2048")
    _, _, ref = engine_for(cfg, precision="f64").run(SEED, 0, 256, ITERS, True, per_trial=True)
    _, _, per = _engine_from(path, cfg).run(SEED, 0, 256, ITERS, True, per_trial=True)
    assert ref.sum() > 0
    assert_counts_equal(per, ref, f"{switch}={other}")
