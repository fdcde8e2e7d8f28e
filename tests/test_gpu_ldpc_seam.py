"""The coded mode's LDPC decoder through its seam (mimo_ldpc_decode) against the numpy reference
(tests/ldpc_ref.py): the final L of every bit, equal element for element.

The inputs of the decoding cases are what the coded mode feeds the decoder: odd integers
``c = 2 clamp(floor(x), -32, 31) + 1`` of a noisy all-zero codeword, ``x = mu + sigma n`` with n
standard normal, at a level (mu, sigma per code below) where the reference decodes some frames and
fails on others -- asserted on the reference alone, before the device is looked at.
"""
import functools

import numpy as np
import pytest

import _engine
import ldpc_ref
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu


def punched_128():
    """z 128, 4 x 8 with four entries punched to -1: rows of weight 7, 7, 8 and 6 (multi-wave layers,
    irregular rows; every column keeps weight >= 3)."""
    s = np.array(qc_ldpc_code(128, 4, 8).table)
    for r, c in ((0, 1), (1, 4), (3, 2), (3, 6)):
        s[r, c] = -1
    return s


# name -> (z, shift table, codewords, mu, sigma)
CODES = {
    "z16_3x6": (16, lambda: qc_ldpc_code(16, 3, 6).table, 48, 4.0, 3.2),       # less than a wave
    "z61_3x6": (61, lambda: qc_ldpc_code(61, 3, 6).table, 24, 4.0, 3.2),       # odd, not a power of two
    "z64_4x8": (64, lambda: qc_ldpc_code(64, 4, 8).table, 24, 4.0, 3.2),
    "z128_4x8_punched": (128, punched_128, 16, 4.0, 3.2),                      # multi-wave layers, irregular rows
    "z512_12x24": (512, lambda: qc_ldpc_code(512, 12, 24).table, 2, 4.0, 2.6),  # the largest state: 73,824 B of LDS
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(shift table, channel values [n_cw, N] int8) of a code; the values are drawn once."""
    z, table, n_cw, mu, sigma = CODES[name]
    s = np.array(table())
    rng = np.random.default_rng(sum(map(ord, name)))
    x = mu + sigma * rng.standard_normal((n_cw, z * s.shape[1]))
    chan = (2 * np.clip(np.floor(x), -32, 31).astype(np.int64) + 1).astype(np.int8)
    chan.setflags(write=False)
    return s, chan


@functools.lru_cache(maxsize=None)
def ref_L(name, iters):
    s, chan = case(name)
    L = ldpc_ref.decode(ldpc_ref.Code(CODES[name][0], s, iters), chan)
    L.setflags(write=False)
    return L


def test_the_decoding_cases_are_not_trivially_clean():
    """On the reference alone: over the cases at least one frame fails and at least one frame with
    channel errors is corrected (10 iterations)."""
    failed = corrected = 0
    for name in CODES:
        _, chan = case(name)
        wrong = (ref_L(name, 10) < 0).any(axis=1)
        failed += int(wrong.sum())
        corrected += int((~wrong & (chan < 0).any(axis=1)).sum())
        print(name, "frames", len(wrong), "failed", int(wrong.sum()), "raw errors", int((chan < 0).sum()))
    assert failed >= 1 and corrected >= 1, (failed, corrected)


@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("name", sorted(CODES))
def test_decoder_equals_the_reference_element_for_element(name, iters):
    s, chan = case(name)
    code = _engine.LdpcCode(CODES[name][0], s, iters)
    L = _engine.ldpc_decode(code, chan)
    assert L.dtype == np.int16 and L.shape == chan.shape
    np.testing.assert_array_equal(L, ref_L(name, iters), err_msg=f"{name}, {iters} iterations")
    # a second call: the same values (no state left behind)
    np.testing.assert_array_equal(_engine.ldpc_decode(code, chan), L)


def test_sign_flip_symmetry_on_the_device():
    """decode(c (-1)^x) == decode(c) (-1)^x for a non-zero codeword x of the z 16, 3 x 6 code and random
    c in [-63, 63], zeros and even values included."""
    from test_coded_host import nonzero_codeword
    table = qc_ldpc_code(16, 3, 6).table
    x = nonzero_codeword(ldpc_ref.Code(16, table))
    flip = 1 - 2 * x.astype(np.int64)
    rng = np.random.default_rng(5)
    c = rng.integers(-63, 64, (40, 96))
    c[:, ::7] = 0
    for iters in (1, 10):
        code = _engine.LdpcCode(16, table, iters)
        plain = _engine.ldpc_decode(code, c)
        np.testing.assert_array_equal(plain, ldpc_ref.decode(ldpc_ref.Code(16, table, iters), c))
        np.testing.assert_array_equal(_engine.ldpc_decode(code, c * flip), plain.astype(np.int64) * flip)


@pytest.mark.parametrize("name", ["z16_3x6", "z512_12x24"])
def test_saturated_input_reaches_the_bound_of_L(name):
    """|c| = 63 everywhere: every message saturates at 127, so |L| reaches 63 + 127 (the bit's
    checks) and stays within 63 + 127 n_rows; all +63, and a random pattern of +-63."""
    z, table, _, _, _ = CODES[name]
    s = np.array(table())
    code = _engine.LdpcCode(z, s, 10)
    ref = ldpc_ref.Code(z, s, 10)
    n = z * s.shape[1]
    rng = np.random.default_rng(9)
    chan = np.stack([np.full(n, 63), np.where(rng.random(n) < 0.5, 63, -63)]).astype(np.int8)
    L = _engine.ldpc_decode(code, chan)
    np.testing.assert_array_equal(L, ldpc_ref.decode(ref, chan))
    assert np.all(L[0] == 63 + 127 * s.shape[0])          # every column has all its blocks
    assert np.abs(L).max() <= 63 + 127 * s.shape[0] <= 8191


def test_no_codewords_is_ok():
    out = _engine.ldpc_decode(qc_ldpc_code(16, 3, 6), np.zeros((0, 96), np.int8))
    assert out.shape == (0, 96)
