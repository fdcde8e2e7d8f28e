"""Counts parity of the float64 wave-split instances where csrc/tuning.h's pass-1 and vk hand-off
switches act (MIMO_P1_HOIST, MIMO_P1_SUMS3, MIMO_VK_LDS): perfect-CSI Rayleigh, soft limiter,
CNC receiver, against oracle/sim.py, per trial and exactly.

Shapes (A, S, F), the smallest that run the changed code:
  (3, 512, 1024)   F 512 runs a one-wave team in float64 (trial_launch.h team_size64: T = 64), so it
                   is not wave-split; F 1024 is the smallest that is: T = 128, two waves, four
                   aligned slots (S % 4T == 0), one region of vk partials;
  (5, 1024, 2048)  the bench instance (T = 256, four waves, three regions), 8 trials.
A = 3 and 5: the alpha wave a mod W wraps and A is no multiple of W.

run_points with two points that differ in IBO: the alpha polynomial differs per team while every
team uses its own partials buffer.

One case per switch at its other value (the project's rule that a switch never changes counts): a
variant library built by
    make -C csrc variant VOUT=../../abl/lib_<SWITCH>_<value>.so VFLAGS=-D<SWITCH>=<value>
gives the default library's counts on 256 trials of the second shape; skipped where that library
was not built."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from gpu_util import assert_counts_equal, engine_for
from oracle import refmath as rm
from oracle import sim

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING = os.path.join(REPO, "m-mimo-ofdm-with-nonlinear-pa-sim_amd", "csrc", "tuning.h")
SHAPES = {"F1024": (3, 512, 1024, 16, 16), "F2048": (5, 1024, 2048, 64, 8)}  # A, S, F, M, trials
ITERS = [0, 1, 2]
SEED = 4242
IBO_B = 1.5  # the second point of the run_points case


def _cfg(shape, ibo=3.0):
    a, s, f, m, _ = SHAPES[shape]
    return sim.SimConfig(a, s, f, m, pa="softlim", ibo_db=ibo, snr_db=16.0)


def _point_of(cfg):
    pp = sim.point_params(cfg)
    return dict(ibo_db=cfg.ibo_db, snr_db=cfg.snr_db, avg_symbol_power=pp["es"], pa_kind=cfg.pa,
                sat_pow=rm.sat_pow(cfg.ibo_db, pp["avg_samp"] / cfg.n_ant), cnc_pa_kind=cfg.pa,
                cnc_sat_pow=pp["cnc_sat"], cnc_alpha=pp["cnc_alpha"])


@functools.lru_cache(maxsize=None)
def _oracle(shape, ibo, seed, first):
    n = SHAPES[shape][4]
    ref = sim.run_trials(_cfg(shape, ibo), seed, np.arange(first, first + n), iters=ITERS, incl_clean=True)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("shape", list(SHAPES))
def test_counts_equal_oracle(shape):
    eng = engine_for(_cfg(shape), precision="f64")
    desc = eng.describe()
    assert "f64" in desc and "aligned" in desc, desc
    _, _, per = eng.run(SEED, 0, SHAPES[shape][4], ITERS, True, per_trial=True)
    ref = _oracle(shape, 3.0, SEED, 0)
    print(f"PASS1_SUMS|{shape}|{desc}|gpu={per.sum(0).tolist()}|oracle={ref.sum(0).tolist()}")
    assert ref.sum() > 0
    assert_counts_equal(per, ref, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_ibo_points_in_one_launch(shape):
    n = SHAPES[shape][4]
    eng = engine_for(_cfg(shape), precision="f64")
    pts = [_point_of(_cfg(shape, 3.0)), _point_of(_cfg(shape, IBO_B))]
    err, _, per = eng.run_points(pts, [SEED, SEED + 1], [0, 5], [n, n], ITERS, True, per_trial=True)
    assert_counts_equal(per[:n], _oracle(shape, 3.0, SEED, 0), f"{shape} IBO 3")
    assert_counts_equal(per[n:], _oracle(shape, IBO_B, SEED + 1, 5), f"{shape} IBO {IBO_B}")
    np.testing.assert_array_equal(err[0], per[:n].sum(0))
    np.testing.assert_array_equal(err[1], per[n:].sum(0))


def _default_of(switch):
    with open(TUNING) as f:
        return int(re.search(r"#define %s (\d+)" % switch, f.read()).group(1))


def _engine_from(path, cfg):
    """An engine of another build of the library (tools/ab_libs.py's way: a variant exports the
    plain run calls only), the binding's own library left as it was."""
    import _engine
    saved = _engine._lib, _engine.LIB_PATH, dict(_engine.SYMBOLS)
    try:
        probe = ctypes.CDLL(path)
        for name in [n for n in saved[2] if not hasattr(probe, n)]:
            del _engine.SYMBOLS[name]
        _engine._lib, _engine.LIB_PATH = None, path
        return engine_for(cfg, precision="f64")
    finally:
        _engine._lib, _engine.LIB_PATH = saved[0], saved[1]
        _engine.SYMBOLS.clear()
        _engine.SYMBOLS.update(saved[2])


@pytest.mark.parametrize("switch", ["MIMO_P1_HOIST", "MIMO_P1_SUMS3", "MIMO_VK_LDS"])
def test_switch_keeps_counts(switch):
    other = 1 - _default_of(switch)
    path = os.path.join(REPO, "abl", f"lib_{switch}_{other}.so")
    if not os.path.exists(path):
        pytest.skip(f"variant library {os.path.relpath(path, REPO)} not built (make -C csrc variant)")
    cfg = _cfg("F2048")
    _, _, ref = engine_for(cfg, precision="f64").run(SEED, 0, 256, ITERS, True, per_trial=True)
    _, _, per = _engine_from(path, cfg).run(SEED, 0, 256, ITERS, True, per_trial=True)
    assert ref.sum() > 0
    assert_counts_equal(per, ref, f"{switch}={other}")
