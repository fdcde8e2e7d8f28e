"""The float64 wave-split instances with their transforms' LDS and twiddle addresses held across the
antenna loop (csrc/tuning.h MIMO_XADDR, MIMO_XADDR_TW; csrc/wave_fft.h XAddr): counts against
oracle/sim.py, per trial and exactly.  Only addresses changed, so nothing may move.

Shapes (A, S, F): those of tests/test_gpu_wave_balance.py, the smallest that reach the changed code:
  (1, 512, 1024), (3, 512, 1024)  the two-wave team (one row pair, NB = 4, stage twiddles, not the
                                  cot-tan form), 16 trials each;
  (5, 1024, 2048)                 the bench instance (four waves; waves 1-3 take the forward
                                  transform's twiddle branch), 8 trials.
CNC iterations 0, 1, 2 and the clean column.  One MCNC case at the bench shape: its later passes
reuse the words held since the main pass.  LoS cases at both sizes: another Channel, the same
transforms.  (The plain Rayleigh instance of F 1024 is one of those that keep re-deriving, since
its scratch would grow, csrc/trial_kernel.h xaddr_inst_ok: at F 1024 it is the LoS case that runs
the held addresses of the two-wave team.)  These shapes are the smallest that reach the changed code,
not all the instances it was compiled into: every other float64 instance of the two sizes -- generic
bands, two-path and table channels, CSI, the six row modes, held or re-deriving -- runs in
tests/test_gpu_wave_split_instances.py (the matrix of tests/wave_split_cases.py).

Switch parity: for each switch a variant library with it off,
    make -C csrc variant VOUT=../../abl/lib_<SWITCH>_0.so VFLAGS=-D<SWITCH>=0
gives the default library's per-trial counts on 256 trials of the bench shape, and on 4 trials its
measure rows are bit for bit the default library's; skipped where that library is not built."""
import functools
import os

import numpy as np
import pytest

from gpu_util import assert_counts_equal, engine_for
from oracle import sim
from test_gpu_pass1_sums import REPO, _engine_from
from test_gpu_wave_balance import ITERS, SEED, SHAPES, _cfg, _default_of, _oracle

pytestmark = pytest.mark.gpu

SWITCHES = ["MIMO_XADDR", "MIMO_XADDR_TW"]
MEAS_TRIALS = 4


@pytest.mark.parametrize("shape", list(SHAPES))
def test_counts_equal_oracle(shape):
    eng = engine_for(_cfg(shape), precision="f64")
    desc = eng.describe()
    assert "f64" in desc and "aligned" in desc, desc
    _, _, per = eng.run(SEED, 0, SHAPES[shape][4], ITERS, True, per_trial=True)
    ref = _oracle(shape, 3.0, SEED, 0)
    print(f"XADDR|{shape}|{desc}|gpu={per.sum(0).tolist()}|oracle={ref.sum(0).tolist()}")
    assert ref.sum() > 0
    assert_counts_equal(per, ref, shape)


def test_mcnc_counts_equal_oracle():
    shape = "F2048"
    eng = engine_for(_cfg(shape, receiver="mcnc"), precision="f64")
    _, _, per = eng.run(SEED, 0, SHAPES[shape][4], ITERS, False, per_trial=True)
    ref = _oracle(shape, 3.0, SEED, 0, "mcnc", False)
    print(f"XADDR|mcnc|{eng.describe()}|gpu={per.sum(0).tolist()}|oracle={ref.sum(0).tolist()}")
    assert ref.sum() > 0
    assert_counts_equal(per, ref, "mcnc")


@functools.lru_cache(maxsize=None)
def _los(shape):
    a, s, f, m, n = SHAPES[shape]
    cfg = sim.SimConfig(a, s, f, m, pa="softlim", ibo_db=3.0, snr_db=16.0, channel="los")
    ref = sim.run_trials(cfg, SEED, np.arange(n), iters=ITERS, incl_clean=True)
    ref.setflags(write=False)
    return cfg, ref


@pytest.mark.parametrize("shape", ["F1024", "F2048"])
def test_los_counts_equal_oracle(shape):
    cfg, ref = _los(shape)
    eng = engine_for(cfg, precision="f64")
    desc = eng.describe()
    assert "f64" in desc and "aligned" in desc and "ch=2" in desc, desc  # the line-of-sight instance
    _, _, per = eng.run(SEED, 0, SHAPES[shape][4], ITERS, True, per_trial=True)
    print(f"XADDR|los|{shape}|{desc}|gpu={per.sum(0).tolist()}|oracle={ref.sum(0).tolist()}")
    assert ref.sum() > 0
    assert_counts_equal(per, ref, f"los {shape}")


def _variant(switch):
    assert _default_of(switch) in (0, 1)
    path = os.path.join(REPO, "abl", f"lib_{switch}_0.so")
    if not os.path.exists(path):
        pytest.skip(f"variant library {os.path.relpath(path, REPO)} not built (make -C csrc variant)")
    return path


@pytest.mark.parametrize("switch", SWITCHES)
def test_switch_keeps_counts(switch):
    path = _variant(switch)
    cfg = _cfg("F2048")
    _, _, ref = engine_for(cfg, precision="f64").run(SEED, 0, 256, ITERS, True, per_trial=True)
    _, _, per = _engine_from(path, cfg).run(SEED, 0, 256, ITERS, True, per_trial=True)
    assert ref.sum() > 0
    assert_counts_equal(per, ref, f"{switch}=0")


@pytest.mark.parametrize("switch", SWITCHES)
def test_switch_keeps_measure_rows_bit_for_bit(switch):
    path = _variant(switch)
    cfg = _cfg("F2048")
    iters = (0, 1)
    _, _, meas, per, rows = engine_for(cfg, precision="f64").measure(SEED, 0, MEAS_TRIALS, iters, False, per_trial=True)
    _, _, vmeas, vper, vrows = _engine_from(path, cfg).measure(SEED, 0, MEAS_TRIALS, iters, False, per_trial=True)
    assert np.all(np.isfinite(rows)) and np.abs(rows).sum() > 0
    assert_counts_equal(vper, per, f"{switch}=0 measure counts")
    assert np.array_equal(vrows, rows), f"{switch}=0: per-trial measure rows differ in {int((vrows != rows).sum())} cells"
    assert np.array_equal(vmeas, meas)
