"""Coded mode of the fused trial kernel (mimo_engine_coded_points) on the GPU: the same counts as the
plain run and the oracle, the channel values of every stream position equal to the oracle-built
reference (tests/ldpc_ref.py) byte for byte, and per trial and counter index the four cells of the
LDPC-decoded link equal to the reference decoder's, cell for cell.

The systems, iteration lists, seeds and ``rho_max`` are tests/test_gpu_soft.py's ``CASES``, by value.
The 64 coded bins are 4 soft bins wide each, so their edges are soft edges at the same ``rho_max``
and the conditions under which the soft histograms compare exactly -- no reliability within the
allowed error of an edge (``near_edge == 0``), none exactly 0 -- hold on these inputs already; every
case still asserts both on the reference before it looks at the device, and that reference cell [0]
is the oracle's error count restricted to the decoded positions.
"""
import dataclasses
import functools

import numpy as np
import pytest

import _engine
import ldpc_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import sim
from test_gpu_ldpc_seam import punched_128
from test_gpu_soft import CASES as SOFT_CASES
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu

N_TRIALS = 8
N_DEC = 10
TABLES = {
    "z16": (16, lambda: qc_ldpc_code(16, 3, 6).table),            # N 96
    "z61": (61, lambda: qc_ldpc_code(61, 3, 6).table),            # N 366: odd lifting size
    "z64": (64, lambda: qc_ldpc_code(64, 4, 8).table),            # N 512
    "z128": (128, punched_128),                                   # N 1,024: multi-wave layers, irregular rows
    "z512": (512, lambda: qc_ldpc_code(512, 12, 24).table),       # N 12,288: the largest state
}
# case -> (soft case, code, decoded bits, n_cw): every variant of the soft cases that the issue lists
CASES = {
    "f128_qpsk-z16": ("f128_qpsk", "z16", 96, 1),          # 128 bits: a tail of 32 undecoded bits
    "f256_generic-z16": ("f256_generic", "z16", 576, 6),
    "f256_generic-z61": ("f256_generic", "z61", 366, 1),   # 234 bits left over
    "f256_skip-z16": ("f256_skip", "z16", 576, 6),         # an unrecorded iteration leaves no row and no c
    "f512_csi-z64": ("f512_csi", "z64", 1024, 2),
    "f2048_mcnc-z128": ("f2048_mcnc", "z128", 6144, 6),
    "f4096_rapp-z128": ("f4096_rapp", "z128", 12288, 12),
    "f8192-z512": ("f8192", "z512", 24576, 2),
    "f128_all_idx-z16": ("f128_all_idx", "z16", 192, 2),   # n_idx 33
}
# the issue's totals for f256_generic over [clean, 0, 1, 2]: (raw, bit, frame, syndrome)
ISSUE_TOTALS = {
    "f256_generic-z16": [(10, 0, 0, 0), (24, 0, 0, 0), (169, 0, 0, 0), (262, 18, 2, 2)],
    "f256_generic-z61": [(7, 0, 0, 0), (16, 0, 0, 0), (114, 0, 0, 0), (164, 0, 0, 0)],
}


@functools.lru_cache(maxsize=None)
def codes(key):
    """(the engine's LdpcCode, the reference's Code) of a table."""
    z, table = TABLES[key]
    t = np.array(table())
    return _engine.LdpcCode(z, t, N_DEC), ldpc_ref.Code(z, t, N_DEC)


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS):
    """(config, counts, channel values, rows [n, n_idx, 4], oracle errors at the decoded positions,
    near-edge count, exact zeros) of a case."""
    soft_name, key, _, _ = CASES[name]
    kw, iters, clean, rho_max, seed = SOFT_CASES[soft_name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    out = ldpc_ref.reference(cfg, codes(key)[1], seed, np.arange(first, first + n), iters, rho_max, clean)
    for a in out[:4]:
        a.setflags(write=False)
    return (cfg,) + out


def assert_reference_conditions(name, cfg, counts, chan, rows, dec_err, near, nz):
    """The conditions on the inputs, on the reference alone."""
    _, key, n_dec, n_cw = CASES[name]
    ref_code = codes(key)[1]
    assert near == 0, f"{name}: {near} reliabilities near a bin edge"
    assert nz == 0, f"{name}: {nz} reliabilities are exactly 0"
    assert (ldpc_ref.n_codewords(cfg.n_sc, cfg.constel_size, ref_code), n_cw * ref_code.n_bits) == (n_cw, n_dec)
    assert chan.shape[2] == cfg.n_sc * int(np.log2(cfg.constel_size)) >= n_dec
    assert np.all(chan % 2 != 0) and np.abs(chan).max() <= 63
    # c < 0 is an uncoded bit error: over the whole stream the oracle's count, over the decoded
    # positions cell [0]
    np.testing.assert_array_equal((chan < 0).sum(axis=2), counts, err_msg=f"{name}: negatives vs counts")
    np.testing.assert_array_equal(rows[:, :, 0], dec_err, err_msg=f"{name}: cell 0 vs the oracle's decisions")
    assert np.all(rows[:, :, 1] <= n_dec) and np.all(rows[:, :, 2:] <= n_cw)
    assert np.all(rows[:, :, 3] <= rows[:, :, 2])  # a flagged frame is wrong


@pytest.mark.parametrize("name", sorted(CASES))
def test_coded_rows_chan_and_counts(name):
    soft_name, key, n_dec, n_cw = CASES[name]
    kw, iters, clean, rho_max, seed = SOFT_CASES[soft_name]
    ref = reference(name)
    assert_reference_conditions(name, *ref)
    cfg, ref_counts, ref_chan, ref_rows = ref[:4]
    if name in ISSUE_TOTALS:
        np.testing.assert_array_equal(ref_rows.sum(axis=0), ISSUE_TOTALS[name])
    n_idx = len(iters) + int(clean)
    code = codes(key)[0]
    eng = engine_for(cfg, precision="f64")
    assert eng.coded_codewords(code) == n_cw
    err, bits, coded, per, per_coded, chan = eng.coded(seed, 0, N_TRIALS, iters, code, rho_max, incl_clean=clean,
                                                       per_trial=True, chan=True)
    kernel_ms, decode_ms = eng.kernel_ms, eng.decode_kernel_ms
    assert kernel_ms > 0 and decode_ms > 0 and eng.beam_kernel_ms == 0
    e_run, b_run, per_run = eng.run(seed, 0, N_TRIALS, iters, incl_clean=clean, per_trial=True)
    assert eng.decode_kernel_ms == 0  # 0 after any other call
    print(name, eng.describe(), "counts", per.sum(0), "cells", coded.tolist(), "kernel ms", kernel_ms, "decode ms",
          decode_ms)
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: coded vs run")
    assert_counts_equal(per, ref_counts, f"{name}: coded vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    # the channel values: the reference's, byte for byte
    assert chan.dtype == np.int8 and chan.shape == ref_chan.shape
    np.testing.assert_array_equal(chan, ref_chan, err_msg=f"{name}: channel values")
    # per-trial rows: the reference's, cell for cell
    assert per_coded.shape == ref_rows.shape == (N_TRIALS, n_idx, 4) and coded.shape == (n_idx, 4)
    np.testing.assert_array_equal(per_coded, ref_rows, err_msg=f"{name}: per-trial rows")
    # totals: the column sums, exactly
    np.testing.assert_array_equal(coded, per_coded.sum(axis=0))
    # and the seam on the device's own channel values gives the rows' decisions
    L = _engine.ldpc_decode(code, ldpc_ref.codewords(codes(key)[1], chan[0, 0]))
    assert ((L < 0).sum(), (L < 0).any(axis=1).sum()) == (per_coded[0, 0, 1], per_coded[0, 0, 2])
    eng.close()


def test_the_cases_hold_corrected_and_failed_frames():
    """On the reference alone: frames with channel errors that decode, and frames that do not."""
    rows = reference("f256_generic-z16")[3]
    assert rows[:, :, 2].sum() >= 1 and np.any((rows[:, :, 0] > 0) & (rows[:, :, 2] == 0))


def test_unrecorded_iteration_leaves_no_row_and_no_values():
    """iters (0, 2) against (0, 1, 2) of the same system: indices clean, 0 and 2 are the same."""
    all_, skip = reference("f256_generic-z16"), reference("f256_skip-z16")
    np.testing.assert_array_equal(skip[3], all_[3][:, [0, 1, 3]])
    np.testing.assert_array_equal(skip[2], all_[2][:, [0, 1, 3]])
    kw, iters, clean, rho_max, seed = SOFT_CASES["f256_skip"]
    code = codes("z16")[0]
    eng = engine_for(sim.SimConfig(**kw), precision="f64")
    _, _, tot_a, _, per_a, chan_a = eng.coded(seed, 0, N_TRIALS, (0, 1, 2), code, rho_max, True, True, chan=True)
    _, _, tot_s, _, per_s, chan_s = eng.coded(seed, 0, N_TRIALS, iters, code, rho_max, True, True, chan=True)
    eng.close()
    np.testing.assert_array_equal(per_s, per_a[:, [0, 1, 3]])
    np.testing.assert_array_equal(chan_s, chan_a[:, [0, 1, 3]])
    np.testing.assert_array_equal(tot_s, tot_a[[0, 1, 3]])


def test_coded_points_rows_and_repeatability():
    """The generic system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, one call."""
    name = "f256_generic-z16"
    _, iters, clean, rho_max, seed = SOFT_CASES["f256_generic"]
    code = codes("z16")[0]
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
    err, bits, coded, per, per_coded, chan = eng.coded_points(points, seeds, first, n_trials, iters, code, rho_max,
                                                              clean, True, chan=True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, clean, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "coded_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[1] for r in refs]), "coded_points vs oracle")
    np.testing.assert_array_equal(chan, np.concatenate([r[2] for r in refs]))
    np.testing.assert_array_equal(per_coded, np.concatenate([r[3] for r in refs]))
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(3):
        own = per_coded[off[i]:off[i + 1]]
        np.testing.assert_array_equal(coded[i], own.sum(axis=0))
        # every point's rows and totals are those of a single-point call, bit for bit
        _, _, c1, _, pc1 = eng.coded(seeds[i], first[i], n_trials[i], iters, code, rho_max, clean, True,
                                     point=points[i])
        np.testing.assert_array_equal(pc1, own)
        np.testing.assert_array_equal(c1, coded[i])
    # a second identical call: bit-identical totals, rows and channel values
    out2 = eng.coded_points(points, seeds, first, n_trials, iters, code, rho_max, clean, True, chan=True)
    np.testing.assert_array_equal(out2[2], coded)
    np.testing.assert_array_equal(out2[4], per_coded)
    np.testing.assert_array_equal(out2[5], chan)
    eng.close()


def test_coded_totals_across_slices_and_launches(monkeypatch):
    """More trials than one reduction slice (4096), and a call split into several launches
    (MIMO_MAX_LAUNCH_TRIALS): the totals are the per-trial rows' sums, and rows, channel values,
    counts and totals do not depend on the splitting."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=25.0)
    code = codes("z16")[0]   # 768 bits: 8 codewords a trial
    eng = engine_for(cfg, precision="f64")
    n = 4096 + 37
    err, _, coded, per, pc, chan = eng.coded(7, 0, n, (0, 1), code, 16.0, per_trial=True, chan=True)
    np.testing.assert_array_equal(coded, pc.sum(axis=0))
    np.testing.assert_array_equal(err, per.sum(0))
    np.testing.assert_array_equal(coded[:, 0], err)          # every position is decoded here
    np.testing.assert_array_equal((chan < 0).sum(axis=2), per)
    assert np.all(coded[:, 1] <= coded[:, 0]) and np.all(coded[:, 3] <= coded[:, 2]) and coded[:, 2].max() <= 8 * n
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "1500")
    err3, _, coded3, per3, pc3, chan3 = eng.coded(7, 0, n, (0, 1), code, 16.0, per_trial=True, chan=True)
    np.testing.assert_array_equal(pc3, pc)
    np.testing.assert_array_equal(chan3, chan)
    np.testing.assert_array_equal(per3, per)
    np.testing.assert_array_equal(err3, err)
    np.testing.assert_array_equal(coded3, coded)
    monkeypatch.delenv("MIMO_MAX_LAUNCH_TRIALS")
    _, _, coded4, _, pc4 = eng.coded(7, 0, n, (0, 1), code, 16.0, per_trial=True)
    np.testing.assert_array_equal(coded4, coded)
    np.testing.assert_array_equal(pc4, pc)
    eng.close()


def test_link_coded_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM, soft limiter at IBO 1: 256 bits a trial
    link.set_snr(14.0)
    code = codes("z16")[0]
    nominal = link.nominal_llr_scale()
    st = link.coded(True, True, [0, 1, 2], [11, 22, 33], N_TRIALS, code)
    assert (st.n_idx, st.n_frames, st.n_code_bits, st.n_bits) == (4, 2 * N_TRIALS, 96, 192 * N_TRIALS)
    eng = link.engine()
    err, bits, coded, _, _ = eng.coded(_seed64([11, 22, 33]), 0, N_TRIALS, [0, 1, 2], code, 32.0 / nominal,
                                       incl_clean=True, point=link.point_params())
    np.testing.assert_array_equal(st.cells, coded)
    np.testing.assert_array_equal(st.raw_ber(), coded[:, 0] / (192 * N_TRIALS))
    # coded_points at two IBOs: point 0 is the call above
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.coded_points(True, True, [0, 1, 2], [[11, 22, 33], [5]], [p0, p1], N_TRIALS, code)
    np.testing.assert_array_equal(both[0].cells, st.cells)
    assert both[1].n_frames == st.n_frames
