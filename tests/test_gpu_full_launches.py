"""The run calls at real launch sizes, and the totals they add to (include/mimo_engine.h).

Launch splitting is otherwise tested scaled down through MIMO_MAX_LAUNCH_TRIALS.  Here nothing is
scaled: on the tiny system of tests/limit_cases.py (1 antenna, 4 sub-carriers, F 128)

* a plain run of 2^20 + 3 trials -- a full launch of 2^20 blocks, 257 reduction slices, and a
  second launch of 3 -- in both precisions: float64 rows EXACTLY the oracle's at the edges of a
  slice and of the launch, at 64 sampled offsets and at the end; totals the column sums;
  bit-identical to two calls split at the seam
* two points of 2^20 - 2 and 7 trials with different seeds and IBOs, the second straddling the
  launch boundary: rows and totals those of one-point calls
* measure mode over the same trials: totals the rows' fsum, sampled rows within
  measure_ref.row_bounds, repeated totals bit-identical
* spectrum mode over its own launch bound MIMO_SPEC_BUFFER_BYTES / (8 n_spec) = 256,140 trials
  plus 5: the plain run's counts, totals those of two calls split at the bound

and on the two-path system D4, for each of the five run calls: err_out, bits_out and the double
totals are ADDED to (counters above 2^32, twice), the per-trial outputs overwritten.

Durations: profiles/r15/limits/README.md.
"""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest

import limit_cases as lc
import measure_ref
from gpu_util import PRECISIONS, assert_counts_equal, assert_f32_counts_close, engine_for

pytestmark = pytest.mark.gpu

N = lc.LAUNCH + 3       # trials of the full-launch calls
FIRST = 5               # their first trial
ITERS = lc.TINY_ITERS
BITS_PER_TRIAL = 16     # 4 sub-carriers of 16-QAM


@functools.lru_cache(maxsize=None)
def plain_run(prec):
    """(err, bits, per-trial counts [N, 3]) of the one call of N trials from FIRST, with clean;
    run once per precision, read-only."""
    eng = engine_for(lc.tiny_config(), precision=prec)
    out = eng.run(lc.TINY_SEED, FIRST, N, ITERS, True, per_trial=True)
    eng.close()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def checked_offsets():
    """The edges of a slice and of a launch, 64 sampled offsets, the last row; and the oracle's
    rows at trial FIRST + offset."""
    off = np.unique(np.concatenate([lc.TINY_OFFSETS, lc.sample_offsets(N), [N - 1]]))
    ref = lc.tiny_rows(FIRST + off)
    ref.setflags(write=False)
    off.setflags(write=False)
    return off, ref


@pytest.mark.parametrize("prec", PRECISIONS)
def test_one_call_of_a_full_launch_and_three_trials(prec):
    err, bits, per = plain_run(prec)
    off, ref = checked_offsets()
    assert per.shape == (N, 3) and set(lc.TINY_OFFSETS) <= set(off.tolist()) and off[-1] == N - 1 and len(off) >= 70
    got = np.asarray(per[off], np.int64)
    print(f"LIMITS_FULL_LAUNCH prec={prec} totals={err.tolist()} agreement_at_{len(off)}_rows={(got == ref).mean():.4f}")
    if prec == "f64":
        assert_counts_equal(got, ref, "full launch f64 vs oracle")
    else:
        assert_f32_counts_close(got, ref, "full launch f32 vs oracle")
    np.testing.assert_array_equal(err, per.astype(np.uint64).sum(0))
    assert err.min() > N // 4  # no column is empty: about one error per trial
    assert all(int(b) == N * BITS_PER_TRIAL for b in bits)
    # the same trials as two calls split at the launch seam
    eng = engine_for(lc.tiny_config(), precision=prec)
    err_a, bits_a, per_a = eng.run(lc.TINY_SEED, FIRST, lc.LAUNCH, ITERS, True, per_trial=True)
    err_b, bits_b, per_b = eng.run(lc.TINY_SEED, FIRST + lc.LAUNCH, 3, ITERS, True, per_trial=True)
    eng.close()
    assert np.array_equal(per[:lc.LAUNCH], per_a) and np.array_equal(per[lc.LAUNCH:], per_b)
    np.testing.assert_array_equal(err, err_a + err_b)
    np.testing.assert_array_equal(bits, bits_a + bits_b)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_a_point_straddles_the_launch_boundary(prec):
    """2^20 - 2 trials of one point and 7 of another (seed and IBO differ): the second point's
    segment is 2 blocks at the end of the first launch and 5 at the start of the second.  Rows and
    totals are those of one-point calls; float64: the 7 rows are the oracle's."""
    n = [lc.LAUNCH - 2, 7]
    seeds, first, ibos = [lc.TINY_SEED, 11], [FIRST, 100], [-2.0, 1.0]
    points = []
    for ibo in ibos:
        e = engine_for(lc.tiny_config(ibo), precision=prec)
        points.append(dict(e.point_kw))
        e.close()
    eng = engine_for(lc.tiny_config(), precision=prec)
    err, bits, per = eng.run_points(points, seeds, first, n, ITERS, True, per_trial=True)
    assert per.shape == (sum(n), 3) and err.shape == (2, 3)
    start = 0
    for i in range(2):
        e1, b1, p1 = eng.run_points([points[i]], [seeds[i]], [first[i]], [n[i]], ITERS, True, per_trial=True)
        assert np.array_equal(per[start:start + n[i]], p1), f"point {i}: rows differ from its one-point call"
        np.testing.assert_array_equal(err[i], e1[0])
        np.testing.assert_array_equal(bits[i], b1[0])
        np.testing.assert_array_equal(err[i], p1.astype(np.uint64).sum(0))
        assert all(int(b) == n[i] * BITS_PER_TRIAL for b in bits[i])
        start += n[i]
    eng.close()
    # point 0 is the head of the one-call run
    assert np.array_equal(per[:n[0]], plain_run(prec)[2][:n[0]])
    ref = lc.tiny_rows(np.arange(100, 107), seed=11, ibo_db=1.0)
    print(f"LIMITS_SEAM prec={prec} second point gpu={per[n[0]:].tolist()} oracle={ref.tolist()}")
    if prec == "f64":
        assert_counts_equal(per[n[0]:], ref, "the straddling point vs oracle")


def test_measure_over_a_full_launch():
    """Measure mode, N trials with per-trial rows (7 columns, 58 MB): counts the plain run's,
    totals the rows' fsum to 1e-12, sampled rows within measure_ref.row_bounds, a repeated call
    bit-identical."""
    err_run, bits_run, per_run = plain_run("f64")
    eng = engine_for(lc.tiny_config(), precision="f64")
    err, bits, meas, per, per_meas = eng.measure(lc.TINY_SEED, FIRST, N, ITERS, False, per_trial=True)
    _, _, meas2, _, _ = eng.measure(lc.TINY_SEED, FIRST, N, ITERS, False)
    eng.close()
    assert per_meas.shape == (N, 7) and per_meas.nbytes == N * 56
    assert np.array_equal(per, per_run[:, 1:])
    np.testing.assert_array_equal(err, err_run[1:])
    np.testing.assert_array_equal(bits, bits_run[1:])
    assert np.all(np.isfinite(per_meas))
    np.testing.assert_allclose(meas, [math.fsum(c) for c in per_meas.T], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(meas2, meas)
    off, _ = checked_offsets()
    ref_counts, ref_rows, ez = measure_ref.reference_rows(lc.tiny_config(), lc.TINY_SEED, FIRST + off, ITERS, False,
                                                          chunk=64)
    assert_counts_equal(per[off], ref_counts, "measure rows' counts vs oracle")
    ratio = np.abs(per_meas[off] - ref_rows) / measure_ref.row_bounds(ref_rows, ez)
    print(f"LIMITS_FULL_MEASURE worst ratio to bound {ratio.max():.3e} over {len(off)} rows")
    assert ratio.max() <= 1.0, f"a measure row deviates {ratio.max():.3g} x its bound"


# ---------------------------------------------------------------- the C calls, caller-owned arrays
def _p(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype)) if a is not None else None


def c_call(eng, name, points, seeds, first, n_trials, iters, clean, err, bits, per=None, probes=None, tot=None,
           rows=None):
    """One call of a run entry point through the bare library with the caller's own output
    arrays (``Engine``'s methods always pass zeros).  ``points``: make_point keywords."""
    import _engine
    L = _engine.lib()
    it = np.ascontiguousarray(iters, np.int32)
    common = [_p(it, ctypes.c_int32), len(it), int(clean), _p(err, ctypes.c_uint64), _p(bits, ctypes.c_uint64),
              _p(per, ctypes.c_uint32)]
    if name == "mimo_engine_run":
        rc = L.mimo_engine_run(eng._h, int(seeds[0]), int(first[0]), int(n_trials[0]), *common)
    else:
        arr = (_engine.MimoPoint * len(points))(*[_engine.Engine.make_point(**kw) for kw in points])
        sd, ft, nt = (np.ascontiguousarray(v, np.uint64) for v in (seeds, first, n_trials))
        args = [eng._h, len(points), arr, _p(sd, ctypes.c_uint64), _p(ft, ctypes.c_uint64), _p(nt, ctypes.c_uint64)]
        tail = []
        if name == "mimo_engine_beam_points":
            pr = np.ascontiguousarray(probes, np.float64)
            tail = [_p(pr, ctypes.c_double), len(pr)]
        if name != "mimo_engine_run_points":
            tail += [_p(tot, ctypes.c_double), _p(rows, ctypes.c_double)]
        rc = getattr(L, name)(*args, *common, *tail)
    assert rc == 0, (name, rc, L.mimo_last_error().decode())


def test_spectrum_over_its_launch_bound():
    """Spectrum mode: a launch holds B = MIMO_SPEC_BUFFER_BYTES // (8 n_spec) = 256,140 trials at
    n_fft 128 (no environment variable lowers it).  One call of B + 5 trials, per-trial counts but no
    per-trial rows: the counts are the plain run's, the totals those of two calls split at B to
    1e-12 of each column's magnitude sum, the radiated power positive and finite."""
    import _engine
    width = _engine.lib().mimo_spectrum_width(128)
    assert width == 128 + lc.SPEC_FIXED
    B = lc.SPEC_BUFFER_BYTES // (8 * width)
    assert B == 256140
    n = B + 5
    cfg = lc.tiny_config()
    eng = engine_for(cfg, precision="f64")
    err, bits = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    per = np.full((n, 3), 0xFFFFFFFF, np.uint32)
    spec = np.zeros(width)
    c_call(eng, "mimo_engine_spectrum_points", [eng.point_kw], [lc.TINY_SEED], [FIRST], [n], ITERS, True, err, bits, per,
           tot=spec)
    _, _, spec_a, _, _ = eng.spectrum(lc.TINY_SEED, FIRST, B, ITERS, True)
    _, _, spec_b, _, _ = eng.spectrum(lc.TINY_SEED, FIRST + B, 5, ITERS, True)
    eng.close()
    per_run = plain_run("f64")[2]
    assert np.array_equal(per, per_run[:n])
    np.testing.assert_array_equal(err, per_run[:n].astype(np.uint64).sum(0))
    assert all(int(b) == n * BITS_PER_TRIAL for b in bits)
    # psd and Ex are sums of non-negative terms, so |a| + |b| is their magnitude sum; for Re C and
    # Im C it is at most that: the bound asked is no wider than 1e-12 of the magnitude sum
    dev = np.abs(spec - (spec_a + spec_b))
    tol = 1e-12 * (np.abs(spec_a) + np.abs(spec_b))
    print(f"LIMITS_FULL_SPECTRUM B={B} worst deviation / tolerance {np.max(dev / tol):.3e} sum(psd)={spec[:128].sum():.6e}")
    assert np.all(dev <= tol), (dev / tol).max()
    psd = spec[:128]
    assert np.all(np.isfinite(spec)) and np.all(psd >= 0) and psd.sum() > 0
    assert spec[128] > 0  # Ex


# ---------------------------------------------------------------- totals are added to
ADD_TRIALS = 5
ADD_ITERS = [0, 1]
ENTRY_POINTS = ["mimo_engine_run", "mimo_engine_run_points", "mimo_engine_measure_points",
                "mimo_engine_spectrum_points", "mimo_engine_beam_points"]
SENTINEL_U32 = 0xDEADBEEF
SENTINEL_F64 = -7.25e300


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_totals_are_added_to_and_per_trial_rows_overwritten(name):
    """D4's system, 5 trials, iterations [0, 1] with clean (run_points: 2 points, IBO 0 and 3).
    err_out starts at 2^33 + 1000 + i, bits_out at 2^40 + i, the double totals at 0.5 + i / 7:
    after a call the integers are the start plus a zero-start call's result, exactly, and the
    doubles np.add(start, that call's totals), bit for bit (one add per element after the
    fixed-order sum); a second call adds again; per-trial outputs lose their sentinel."""
    cfg, _, _ = lc.deep_config("D4")
    eng = engine_for(cfg, precision="f64")
    points = [dict(eng.point_kw)]
    if name == "mimo_engine_run_points":
        other = engine_for(dataclasses.replace(cfg, ibo_db=3.0), precision="f64")
        points.append(dict(other.point_kw))
        other.close()
    P = len(points)
    seeds, first, n = [lc.DEEP_SEED, 43][:P], [0, 9][:P], [ADD_TRIALS, 4][:P]
    n_idx = 1 + len(ADD_ITERS)
    probes = lc.beam_probes() if name == "mimo_engine_beam_points" else None
    width = {"mimo_engine_measure_points": 5 + n_idx, "mimo_engine_spectrum_points": cfg.n_fft + 3,
             "mimo_engine_beam_points": 9 * 5}.get(name)

    def call(err, bits, per, tot, rows):
        c_call(eng, name, points, seeds, first, n, ADD_ITERS, True, err, bits, per, probes=probes, tot=tot, rows=rows)

    def doubles(shape, fill):
        return None if width is None else np.full(shape, fill)

    # the zero-start call: what Engine's methods do
    err0, bits0 = np.zeros(P * n_idx, np.uint64), np.zeros(P * n_idx, np.uint64)
    per0 = np.zeros((sum(n), n_idx), np.uint32)
    tot0, rows0 = doubles(P * (width or 0), 0.0), doubles((sum(n), width or 0), 0.0)
    call(err0, bits0, per0, tot0, rows0)
    ref = lc.deep_reference("D4", tuple(ADD_ITERS), True)[:ADD_TRIALS]
    assert_counts_equal(per0[:ADD_TRIALS], ref, f"{name} vs oracle")
    np.testing.assert_array_equal(err0[:n_idx], ref.sum(0))
    assert err0.min() > 0 and np.all(bits0[:n_idx] == ADD_TRIALS * cfg.n_sc * 4)
    if width is not None:
        assert np.all(np.isfinite(tot0)) and np.abs(tot0).sum() > 0

    i = np.arange(P * n_idx, dtype=np.uint64)
    err = np.uint64(2 ** 33 + 1000) + i
    bits = np.uint64(2 ** 40) + i
    err_start, bits_start = err.copy(), bits.copy()
    tot = None if width is None else 0.5 + np.arange(P * width) / 7
    tot_start = None if width is None else tot.copy()
    expect_tot = tot_start
    for k in (1, 2):
        per = np.full((sum(n), n_idx), SENTINEL_U32, np.uint32)
        rows = doubles((sum(n), width or 0), SENTINEL_F64)
        call(err, bits, per, tot, rows)
        np.testing.assert_array_equal(err, err_start + np.uint64(k) * err0, err_msg=f"{name}: err_out, call {k}")
        np.testing.assert_array_equal(bits, bits_start + np.uint64(k) * bits0, err_msg=f"{name}: bits_out, call {k}")
        assert np.array_equal(per, per0), f"{name}: per-trial counts are not overwritten (call {k})"
        if width is not None:
            expect_tot = np.add(expect_tot, tot0)
            np.testing.assert_array_equal(tot, expect_tot, err_msg=f"{name}: double totals, call {k}")
            assert np.array_equal(rows, rows0), f"{name}: per-trial rows are not overwritten (call {k})"
    assert err.min() > 2 ** 33 and bits.min() > 2 ** 40
    eng.close()
