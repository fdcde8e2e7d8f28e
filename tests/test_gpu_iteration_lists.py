"""The fused trial kernel at the iteration depth the header allows: lists up to iteration 31, the
33-counter rows and the 38-column measure rows (tests/limit_cases.py ``DEEP``).

* float64: the per-trial counts of every case's list, with clean, EXACTLY the oracle's
* sparse lists ([31], [0, 31], [5, 8], 1..8; clean on and off): the same columns of the FULL run,
  bit for bit -- the counter index follows the recorded columns, not the iteration
* measure mode on FULL: the plain run's counts, 38-column rows within measure_ref.row_bounds
* spectrum and beam mode with [0, 31]: the plain run's counts, rows bit-identical to the call
  with [0] -- the receiver's depth does not touch what the array radiates
* float32: the project's criterion (gpu_util.assert_f32_counts_close) on the clean and
  iteration-0 columns of every case and on all columns of the settling cases; in the cycling
  cases one rounding flip feeds back, so their deeper columns are printed (LIMITS_AGREE), not
  asserted

tests/test_limit_cases.py shows on the CPU that consecutive columns of every case differ, so a
loop that stops early cannot pass.  Measured agreement: profiles/r15/limits/README.md.
"""
import functools
import math

import numpy as np
import pytest

import limit_cases as lc
import measure_ref
from gpu_util import PRECISIONS, assert_counts_equal, assert_f32_counts_close, engine_for

pytestmark = pytest.mark.gpu

FULL_COLS = 1 + len(lc.FULL)  # 33 counters


@functools.lru_cache(maxsize=None)
def own_run(tag, prec):
    """(err, bits, per-trial counts, describe()) of the case's own list with clean; run once, read-only."""
    cfg, n, iters = lc.deep_config(tag)
    eng = engine_for(cfg, precision=prec)
    err, bits, per = eng.run(lc.DEEP_SEED, 0, n, iters, True, per_trial=True)
    desc = eng.describe()
    eng.close()
    for a in (err, bits, per):
        a.setflags(write=False)
    return err, bits, per, desc


def bits_of(cfg, n):
    return n * cfg.n_sc * int(np.log2(cfg.constel_size))


@pytest.mark.parametrize("tag", lc.DEEP_TAGS)
def test_float64_counts_to_iteration_31_vs_oracle(tag):
    """Per-trial counts of the case's list (FULL: 33 counters; D6: [0, 8, 31]) EXACTLY the oracle's,
    totals their column sums, bit counts right, and the team describe() names."""
    cfg, n, iters = lc.deep_config(tag)
    ref = lc.deep_reference(tag)
    err, bits, per, desc = own_run(tag, "f64")
    print(f"LIMITS_DESCRIBE {tag} [{desc}] gpu={per.sum(0).tolist()}")
    assert desc == lc.DEEP_DESCRIBE[tag], desc
    assert per.shape == (n, 1 + len(iters)) and (tag == "D6" or per.shape[1] == FULL_COLS)
    assert_counts_equal(per, ref, f"{tag} f64")
    np.testing.assert_array_equal(err, per.astype(np.uint64).sum(0))
    assert all(int(b) == bits_of(cfg, n) for b in bits) and len(bits) == per.shape[1]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("tag", ["D1", "D2", "D3", "D4", "D5"])
def test_sparse_lists_record_the_columns_of_the_full_run(tag, prec):
    """Every list of SPARSE, with and without clean: rows, totals and bit counts are the same
    columns of the FULL run, bit for bit, in both precisions; float64 on D1 and D2 also against an
    oracle run with that list."""
    cfg, n, _ = lc.deep_config(tag)
    err_full, _, full, _ = own_run(tag, prec)
    eng = engine_for(cfg, precision=prec)
    for iters in lc.SPARSE:
        for clean in (True, False):
            cols = lc.columns_of(iters, clean)
            err, bits, per = eng.run(lc.DEEP_SEED, 0, n, iters, clean, per_trial=True)
            label = f"{tag} {prec} iters={iters} clean={clean}"
            assert per.shape == (n, len(cols)), label
            assert_counts_equal(per, full[:, cols], label + " vs the FULL run")
            np.testing.assert_array_equal(err, err_full[cols], err_msg=label)
            assert all(int(b) == bits_of(cfg, n) for b in bits) and len(bits) == len(cols)
            if prec == "f64" and tag in ("D1", "D2"):
                assert_counts_equal(per, lc.deep_reference(tag, tuple(iters), clean), label + " vs oracle")
    eng.close()


@functools.lru_cache(maxsize=None)
def measure_reference(tag):
    cfg, n, iters = lc.deep_config(tag)
    out = measure_ref.reference_rows(cfg, lc.DEEP_SEED, np.arange(n), iters, True, chunk=4)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("tag", ["D1", "D2"])
def test_measure_rows_at_38_columns(tag):
    """Measure mode on FULL plus clean: the plain run's counts, 5 + 33 columns, every row within
    measure_ref.row_bounds (unchanged: 1e-13 relative on z), totals the rows' fsum to 1e-12."""
    cfg, n, iters = lc.deep_config(tag)
    ref_counts, ref_rows, ez = measure_reference(tag)
    np.testing.assert_array_equal(ref_counts, lc.deep_reference(tag))
    err_run, bits_run, per_run, _ = own_run(tag, "f64")
    eng = engine_for(cfg, precision="f64")
    err, bits, meas, per, per_meas = eng.measure(lc.DEEP_SEED, 0, n, iters, True, per_trial=True)
    eng.close()
    assert_counts_equal(per, per_run, f"{tag}: measure vs run")
    np.testing.assert_array_equal(err, err_run)
    np.testing.assert_array_equal(bits, bits_run)
    assert per_meas.shape == ref_rows.shape == (n, 38) and meas.shape == (38,)
    assert np.all(np.isfinite(per_meas))
    ratio = np.abs(per_meas - ref_rows) / measure_ref.row_bounds(ref_rows, ez)
    print(f"LIMITS_MEASURE_RATIO {tag} worst={ratio.max():.3e} fixed={ratio[:, :5].max():.2e} "
          f"clean={ratio[:, 5].max():.2e} it0={ratio[:, 6].max():.2e} it31={ratio[:, 37].max():.2e}")
    assert ratio.max() <= 1.0, f"{tag}: a measure row deviates {ratio.max():.3g} x its bound"
    np.testing.assert_allclose(meas, [math.fsum(c) for c in per_meas.T], rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode", ["spectrum", "beam"])
def test_the_receiver_depth_does_not_touch_what_the_array_radiates(mode):
    """D1 with [0, 31] and clean: the counts are the plain run's columns, and the totals and
    per-trial rows are bit-identical to the same call with [0]."""
    tag = "D1"
    cfg, n, _ = lc.deep_config(tag)
    err_run, _, per_run, _ = own_run(tag, "f64")
    cols = lc.columns_of([0, 31], True)
    eng = engine_for(cfg, precision="f64")
    if mode == "spectrum":
        call = lambda iters: eng.spectrum(lc.DEEP_SEED, 0, n, iters, True, per_trial=True)  # noqa: E731
        shape = (n, cfg.n_fft + 3)
    else:
        probes = lc.beam_probes()
        assert probes.shape == (9, 3)
        call = lambda iters: eng.beam(lc.DEEP_SEED, 0, n, iters, probes, True, per_trial=True)  # noqa: E731
        shape = (n, 9, 5)
    err, bits, tot, per, rows = call([0, 31])
    err0, bits0, tot0, per0, rows0 = call([0])
    eng.close()
    assert_counts_equal(per, per_run[:, cols], f"{mode} [0, 31] vs run")
    np.testing.assert_array_equal(err, err_run[cols])
    assert_counts_equal(per0, per_run[:, cols[:2]], f"{mode} [0] vs run")
    assert rows.shape == rows0.shape == shape and np.all(np.isfinite(rows)) and rows.sum() > 0
    np.testing.assert_array_equal(rows, rows0)
    np.testing.assert_array_equal(tot, tot0)


@pytest.mark.parametrize("tag", lc.DEEP_TAGS)
def test_float32_counts_to_iteration_31(tag):
    """float32 on the same launches: totals are the column sums and the bit counts right in every
    case; the float32 criterion holds on the clean and iteration-0 columns of every case, where no
    feedback has acted yet, and on all columns of the settling cases D2 and D4.  The deeper columns
    of the cycling cases are printed, not asserted: one rounding flip there feeds back."""
    cfg, n, iters = lc.deep_config(tag)
    ref = lc.deep_reference(tag)
    err, bits, per, desc = own_run(tag, "f32")
    per = np.asarray(per, np.int64)
    assert desc.endswith("f32") and per.shape == ref.shape
    agree = (per == ref).mean(0)
    print(f"LIMITS_AGREE {tag} prec=f32 [{desc}] overall={(per == ref).mean():.4f} max_off={int(np.abs(per - ref).max())} "
          f"per_column=" + ",".join(f"{v:.3f}" for v in agree))
    print(f"LIMITS_AGREE {tag} prec=f32 gpu={per.sum(0).tolist()} oracle={ref.sum(0).tolist()}")
    np.testing.assert_array_equal(err, per.astype(np.uint64).sum(0))
    assert all(int(b) == bits_of(cfg, n) for b in bits)
    assert_f32_counts_close(per[:, :2], ref[:, :2], f"{tag} f32 clean and iteration 0")
    if tag in lc.SETTLING:
        assert_f32_counts_close(per, ref, f"{tag} f32 all columns")
