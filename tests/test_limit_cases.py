"""CPU: pins the case tables of tests/limit_cases.py, from the oracle alone.

The conditions are on the inputs of tests/test_gpu_iteration_lists.py, tests/test_gpu_sizes.py and
tests/test_gpu_full_launches.py: a case that misses one gets another seed or Eb/N0, never a
lower threshold.  D1..D5 passed as first tabled (seed 41; Eb/N0 10, 14, 14, 9 and 15 dB).  D6 at its
first Eb/N0, 12 dB, counted [44, 42] errors at iteration 8 and at iteration 31: no difference.  At
10 dB, seed unchanged, the two columns are [143, 137] and [145, 138]; that is the value tabled.
"""
import re

import numpy as np
import pytest

import limit_cases as lc


def test_the_shared_lists():
    assert lc.FULL == list(range(32)) and len(lc.FULL) + 1 == 33
    assert lc.SPARSE == ([31], [0, 31], [5, 8], [1, 2, 3, 4, 5, 6, 7, 8])
    assert lc.columns_of([0, 31], True) == [0, 1, 32] and lc.columns_of([5, 8], False) == [6, 9]
    assert lc.DEEP_SEED == 41 and [lc.DEEP[t][8] for t in lc.DEEP_TAGS] == [12, 12, 12, 12, 3, 2]
    assert lc.deep_config("D6")[2] == [0, 8, 31] and lc.deep_config("D1")[2] is lc.FULL


@pytest.mark.parametrize("tag", lc.SMALL_TAGS)
def test_every_deep_column_is_informative(tag):
    """On FULL, every pair of consecutive iteration columns differs in at least 2 of the 12
    trials, and every iteration column has errors: a kernel that stopped iterating early, at any
    depth, or recorded a column twice, cannot equal the oracle."""
    ref = lc.deep_reference(tag)
    assert ref.shape == (12, 33)
    it = ref[:, 1:]
    differ = (it[:, 1:] != it[:, :-1]).sum(0)
    print("LIMITS_DEEP", tag, "consecutive columns differ in", differ.tolist(), "totals", ref.sum(0).tolist())
    assert differ.min() >= 2, differ.tolist()
    assert np.all(it.sum(0) > 0) and ref[:, 0].sum() > 0
    # the figures of the table's author: columns 30 and 31 differ in this many trials
    assert int((it[:, 30] != it[:, 31]).sum()) == {"D1": 12, "D2": 4, "D3": 12, "D4": 3}[tag]


@pytest.mark.parametrize("tag", ["D5", "D6"])
def test_the_deepest_columns_of_the_large_teams_differ(tag):
    """D5 (iterations 30 and 31) and D6 (8 and 31): the two deepest recorded columns differ in at
    least one trial, and every column has errors."""
    cfg, n, iters = lc.deep_config(tag)
    ref = lc.deep_reference(tag)
    assert ref.shape == (n, 1 + len(iters))
    print("LIMITS_DEEP", tag, "deepest columns", ref[:, -2].tolist(), ref[:, -1].tolist(), "totals", ref.sum(0).tolist())
    assert (ref[:, -2] != ref[:, -1]).sum() >= 1
    assert np.all(ref.sum(0) > 0)


@pytest.mark.parametrize("tag", ["D1", "D2"])
def test_a_sparse_list_is_the_full_run_columns(tag):
    """The oracle itself: a sparse list records the same columns a FULL run does (what
    tests/test_gpu_iteration_lists.py asks of the kernel's ``idx``)."""
    full = lc.deep_reference(tag)
    for iters in lc.SPARSE:
        for clean in (True, False):
            np.testing.assert_array_equal(lc.deep_reference(tag, tuple(iters), clean),
                                          full[:, lc.columns_of(iters, clean)])


@pytest.mark.parametrize("tag", lc.DEEP_TAGS)
def test_the_described_instance_matches_the_table(tag):
    """DEEP_DESCRIBE against the table and the team sizes of csrc/trial_launch.h (float64: 64
    threads below F 512, F / 8 up to F 2048, F / 16 from F 4096): D3 alone runs generic slots."""
    A, S, F, M, ibo, ebn0, channel, receiver, n, own = lc.DEEP[tag]
    m = re.fullmatch(r"F=(\d+) T=(\d+) slots=(\d+) (aligned|generic) ch=(\d) csi=0 f64", lc.DEEP_DESCRIBE[tag])
    f, t, slots, kind, ch = int(m[1]), int(m[2]), int(m[3]), m[4], int(m[5])
    assert f == F and t == (F // 16 if F >= 4096 else F // 8 if F >= 512 else 64)
    aligned = S % (4 * t) == 0 and S // t in (4, 8) and S // t < F // t
    assert kind == ("aligned" if aligned else "generic") and (kind == "generic") == (tag == "D3")
    assert slots == (S // t if aligned else F // t)
    assert ch == {"rayleigh": 1, "two_path": 3}[channel]


@pytest.mark.parametrize("i", lc.LARGE_NUMBERS, ids=lc.large_id)
def test_large_constellation_totals(i):
    """The oracle's totals [clean, it0, it1, it2] of each large-constellation case, as the table
    states them: errors in every column, and the settling cases settle."""
    ref = lc.large_reference(i)
    A, S, F, M, ebn0, receiver, totals = lc.LARGE[i]
    assert ref.shape == (lc.LARGE_TRIALS, 4)
    assert ref.sum(0).tolist() == totals
    assert min(totals) > 0 and max(totals) < 0.25 * lc.LARGE_TRIALS * S * int(np.log2(M))
    assert (i in lc.LARGE_SETTLING) == (receiver == "mcnc") == (totals[3] < totals[1])
    assert int(np.sqrt(M)) - 1 == (63 if M == 4096 else 31)  # the largest lattice level


def test_the_tiny_system_at_the_edges_of_a_slice_and_a_launch():
    cfg = lc.tiny_config()
    assert (cfg.n_ant, cfg.n_sc, cfg.n_fft, cfg.constel_size, cfg.ibo_db) == (1, 4, 128, 16, -2.0)
    assert lc.TINY_OFFSETS == [0, 1, 4095, 4096, 4097, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 2]
    np.testing.assert_array_equal(lc.tiny_rows(lc.TINY_OFFSETS), lc.TINY_ROWS)
    # without the clean column: the same iteration columns
    np.testing.assert_array_equal(lc.tiny_rows(lc.TINY_OFFSETS, incl_clean=False), np.asarray(lc.TINY_ROWS)[:, 1:])
    # another seed or IBO is another system (the two-point launch of the GPU test tells them apart)
    assert (lc.tiny_rows(np.arange(64), seed=11) != lc.tiny_rows(np.arange(64))).any()
    assert (lc.tiny_rows(np.arange(64), ibo_db=1.0) != lc.tiny_rows(np.arange(64))).any()
    # a sample of trials is informative: the three columns differ from each other and vary
    rows = lc.tiny_rows(5 + lc.sample_offsets(lc.LAUNCH + 3))
    assert len(np.unique(rows, axis=0)) >= 8
    assert (rows[:, 0] != rows[:, 1]).any() and (rows[:, 1] != rows[:, 2]).any()


def test_the_sampled_offsets_are_fixed_and_spread():
    off = lc.sample_offsets(lc.LAUNCH + 3)
    assert off.size == 64 == len(set(off.tolist())) and off.min() >= 0 and off.max() < lc.LAUNCH + 3
    np.testing.assert_array_equal(off, lc.sample_offsets(lc.LAUNCH + 3))
    # ... over the reduction slices: the 64 draws fall into at least 48 different slices of 4096
    assert len(set((off // lc.SLICE).tolist())) >= 48


def test_the_spectrum_launch_bound_of_the_tiny_system():
    """MIMO_SPEC_BUFFER_BYTES // (8 (n_fft + MIMO_SPEC_FIXED)) at n_fft 128, from the header's text."""
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "mimo_engine.h")).read()
    assert re.search(r"#define MIMO_SPEC_BUFFER_BYTES \(256u << 20\)", header)
    assert re.search(r"enum \{ MIMO_SPEC_FIXED = 3 \};", header)
    assert lc.SPEC_BUFFER_BYTES // (8 * (128 + lc.SPEC_FIXED)) == 256140
