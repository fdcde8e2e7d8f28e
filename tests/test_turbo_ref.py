"""The turbo mode's reference (tests/turbo_ref.py) on the CPU: pinned to the issue's table -- 8 antennas,
LoS, F 512, S 256, 64-QAM, soft limiter at IBO 0 dB, SNR 20 dB, seed 7, trials 0..7,
``qc_ldpc_code(64, 4, 8)`` at 10 decoder iterations (3 codewords a symbol, no tail), ``rho_max`` 16 --
and checked against the coded mode's reference where the two must agree."""
import functools

import numpy as np

import ldpc_ref
import turbo_ref
from oracle import sim
from utilities import qc_ldpc_code

SEED, N_TRIALS, RHO_MAX, N_PASSES = 7, 8, 16.0, 4
# totals over the 8 trials per pass: (uncoded errors, decoded bit errors, wrong frames, flagged frames)
DECODER_FEEDBACK = [(1191, 102, 3, 3), (183, 0, 0, 0), (144, 0, 0, 0), (144, 0, 0, 0)]
HARD_FEEDBACK = [(1191, 102, 3, 3), (876, 0, 0, 0), (798, 0, 0, 0), (774, 0, 0, 0)]


def config():
    return sim.SimConfig(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", ibo_db=0.0, snr_db=20.0,
                         channel="los")


def code():
    return ldpc_ref.Code(64, np.array(qc_ldpc_code(64, 4, 8).table), 10)


@functools.lru_cache(maxsize=None)
def reference(feedback):
    return turbo_ref.reference(config(), code(), SEED, np.arange(N_TRIALS), RHO_MAX, N_PASSES, feedback=feedback)


@functools.lru_cache(maxsize=None)
def coded_reference():
    return ldpc_ref.reference(config(), code(), SEED, np.arange(N_TRIALS), (0, 1, 2, 3), RHO_MAX)


def test_the_setting_has_three_codewords_and_no_tail():
    assert ldpc_ref.n_codewords(256, 64, code()) == 3 and 3 * code().n_bits == 256 * 6


def test_decoder_feedback_totals_are_the_issues():
    _, chan, rows, _, near, nz = reference("decoder")
    assert (near, nz) == (0, 0)
    np.testing.assert_array_equal(rows.sum(axis=0), DECODER_FEEDBACK)
    np.testing.assert_array_equal((chan[:, :, :3 * 512] < 0).sum(axis=2), rows[:, :, 0])


def test_hard_feedback_totals_are_the_issues():
    np.testing.assert_array_equal(reference("hard")[2].sum(axis=0), HARD_FEEDBACK)


def test_hard_feedback_is_the_coded_reference_per_iteration():
    """Hard slices fed back: pass q is the coded mode at CNC iteration q, rows and channel values."""
    _, chan, rows, _, _, _ = reference("hard")
    _, ref_chan, ref_rows, _, _, _ = coded_reference()
    np.testing.assert_array_equal(rows, ref_rows)
    np.testing.assert_array_equal(chan, ref_chan)


def test_pass_0_is_the_coded_references_iteration_0():
    counts, chan, rows, _, _, _ = reference("decoder")
    ref_counts, ref_chan, ref_rows, _, _, _ = coded_reference()
    np.testing.assert_array_equal(rows[:, 0], ref_rows[:, 0])
    np.testing.assert_array_equal(chan[:, 0], ref_chan[:, 0])
    np.testing.assert_array_equal(counts[:, 0], ref_counts[:, 0])


def test_fixed_point_after_a_pass_that_decodes_every_frame():
    """Pass 1 decodes every frame of every trial and the stream has no tail: the decisions are the
    transmitted labels, so passes 2 and 3 are equal, per trial, in rows and channel values."""
    _, chan, rows, _, _, _ = reference("decoder")
    assert np.all(rows[:, 1, 1:] == 0)
    np.testing.assert_array_equal(rows[:, 2], rows[:, 3])
    np.testing.assert_array_equal(chan[:, 2], chan[:, 3])


def test_decided_labels_are_the_transmitted_ones_where_nothing_is_wrong():
    cfg, c = config(), code()
    labels = np.arange(256) % 64
    chan = np.ones(256 * 6, np.int8)
    L = np.ones((3, 512), np.int16)
    np.testing.assert_array_equal(turbo_ref.decided_labels(cfg, c, labels, chan, L), labels)
    # one decoder decision flipped: bit n of codeword w is stream position 3 n + w = j S + k
    L[1, 100] = -1
    pos = 3 * 100 + 1
    j, k = divmod(pos, 256)
    got = turbo_ref.decided_labels(cfg, c, labels, chan, L)
    want = labels.copy()
    want[k] ^= 1 << (5 - j)
    np.testing.assert_array_equal(got, want)
