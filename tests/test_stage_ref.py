"""The long-double references of tests/stage_ref.py against the float64 oracle
(oracle/refmath.py, oracle/philox.py) on a machine without a GPU: each agrees to float64
rounding, so a slip in a reference (a bin map, a sign, a scale, a Philox word) shows here and
not as a puzzling device error."""
import numpy as np
import pytest

import probe_util as pu
import stage_ref as sr
from oracle import refmath as rm

U = sr.U


def _cnormal(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)


@pytest.mark.parametrize("F,S,cp", [(128, 4, 0), (128, 126, 128), (256, 6, 7), (2048, 1024, 128)])
def test_ofdm_references_agree_with_the_oracle(F, S, cp):
    """Relative l2 <= 2 log2(F) u per row: an FFT's rms error grows no faster than u log2 N."""
    rng = np.random.default_rng(F + S + cp)
    sym = _cnormal(rng, (3, S))
    tx_ld = sr.ld_ofdm_tx(sym, F, S, cp)
    tx_np = rm.ofdm_tx(sym, F, S, cp)
    assert tx_ld.shape == tx_np.shape == (3, F + cp)
    bound = 2 * np.log2(F) * U
    l2, _ = pu.errors(tx_np, tx_ld)
    assert 0 < l2.max() <= bound
    # the prefix is a copy of the body's tail
    assert np.array_equal(tx_ld[:, :cp], tx_ld[:, F:])
    rx_ld = sr.ld_ofdm_rx(tx_np, F, S, cp)
    l2, _ = pu.errors(rm.ofdm_rx(tx_np, F, S, cp), rx_ld)
    assert 0 < l2.max() <= bound
    # rx(tx(s)) = s
    assert pu.errors(sr.ld_ofdm_rx(tx_ld, F, S, cp), sym)[0].max() <= 1e-17 * np.log2(F)


@pytest.mark.parametrize("M,lo", [(4, 0.3), (16, 0.3), (64, 0.3), (256, 2.0)])
def test_llr_reference_agrees_with_the_oracle(M, lo):
    """|llr - ref| / max(1, |ref|) <= 64 u: the exponent x = |z - C|^2 / nv carries a few u of
    relative rounding, exp turns that into a few x u relative, and the LLR (a difference of
    exponents of that size plus a log of sums) keeps it relative to its own size."""
    L = int(np.sqrt(M))
    rng = np.random.default_rng(M)
    z = rng.uniform(-L - 1, L + 1, 257) + 1j * rng.uniform(-L - 1, L + 1, 257)
    nv = rng.uniform(lo, 8.0, 257)
    const = rm.gray_qam_constellation(M)
    want = rm.soft_llr(const, z, nv).reshape(257, -1)
    assert np.all(np.isfinite(want))
    ref = sr.ld_llr(const, z, nv)
    err = np.asarray(np.abs(want - ref) / np.maximum(1, np.abs(ref)), np.float64)
    assert 0 < err.max() <= 64 * U


def test_llr_exponents_name_the_underflow():
    """Where every exponent is above -600 or below -900 the float64 sums' zeros are decided
    far from exp's underflow threshold (-745): the oracle's +-inf pattern is then well defined."""
    const = rm.gray_qam_constellation(16)
    z = np.array([0.9 + 1.1j])
    e = sr.llr_exponents(const, z, 1e-3)
    assert np.all((e > -600) | (e < -900))
    llr = rm.soft_llr(const, z, 1e-3)
    assert np.isinf(llr).any()


@pytest.mark.parametrize("A,K", [(1, 1), (3, 5), (64, 300), (4096, 4)])
def test_mrt_and_combine_references_agree_with_the_oracle(A, K):
    rng = np.random.default_rng(A * 1000 + K)
    h = _cnormal(rng, (A, K)) * 10.0 ** rng.uniform(-3, 3, (A, 1))
    y = _cnormal(rng, (A, K))
    p_ld = sr.ld_mrt(h)
    assert np.all(np.abs(rm.mrt_precoding(h) - p_ld) <= (A / 2 + 4) * U * 1.01 * np.abs(p_ld))
    c_ld, scale = sr.ld_combine(h, y)
    assert np.all(np.abs(np.sum(h * y, axis=0) - c_ld) <= np.sqrt(2) * (A + 2) * U * 1.01 * scale)
    # unit norm per column
    assert np.allclose(np.asarray(np.sum(np.abs(p_ld) ** 2, axis=0), np.float64), 1.0, rtol=1e-15, atol=0)


@pytest.mark.parametrize("seed,counter", [(1, 0), (0x0123456789ABCDEF, 7), (2 ** 63 - 1, 2 ** 32 + 5)])
def test_awgn_reference_agrees_with_the_oracle(seed, counter):
    """Relative to the sample's modulus <= 16 u: the float64 angle 2 pi u2 is off by up to
    about 2 pi (1.5 u) radians (pi's and the product's rounding), the radius by about 2 u."""
    idx = np.concatenate((np.arange(300), sr.GRID_PASS + np.arange(-2, 259), 2 ** 32 + np.arange(3)))
    ref = sr.ld_awgn_noise(seed, counter, idx, 0.37)
    got = sr.np_awgn_noise(seed, counter, idx, 0.37)
    err = np.asarray(np.abs(got - ref) / np.abs(ref), np.float64)
    assert 0 < err.max() <= 16 * U
    # E|n|^2 = std^2 / 2: (x + j y) std / 2 with x, y ~ N(0, 1)  (noise.py:56-83)
    assert np.mean(np.abs(got[:300]) ** 2) == pytest.approx(0.37 ** 2 / 2, rel=0.2)
    # the high halves of seed, counter and index all reach the words
    w = sr.awgn_words(seed, counter, idx)[0]
    assert not np.array_equal(w, sr.awgn_words(seed ^ (1 << 40), counter, idx)[0])
    assert not np.array_equal(w, sr.awgn_words(seed, counter ^ (1 << 32), idx)[0])
    assert sr.awgn_words(seed, counter, [5])[0] != sr.awgn_words(seed, counter, [2 ** 32 + 5])[0]
    # ... and index-high and counter-high share a word: (i, ctr) and (i + 2^32, ctr ^ 2^32) collide by design
    assert sr.awgn_words(seed, counter, [5])[0] == sr.awgn_words(seed, counter ^ (1 << 32), [2 ** 32 + 5])[0]


@pytest.mark.parametrize("F,S,M,pa,p", [(128, 4, 4, "softlim", 0.0), (256, 252, 64, "rapp", 2.5),
                                        (512, 256, 256, "toi", 0.0)])
def test_cnc_reference_agrees_with_the_oracle(F, S, M, pa, p):
    const = rm.gray_qam_constellation(M)
    rng = np.random.default_rng(F + M)
    avg = rm.ofdm_avg_sample_power(const, F, S)
    sat, coeff, alpha = rm.sat_pow(2.0, avg), rm.toi_coeff(12.0, avg), 0.9
    tx = const[rng.integers(0, M, S)]
    up = np.zeros(F, complex)
    up[rm.inband_bins(F, S)] = tx
    rx = np.fft.fft(rm.apply_pa(pa, np.fft.ifft(up, norm="ortho"), sat, p, coeff), norm="ortho")[rm.inband_bins(F, S)]
    rx = rx / alpha + 0.05 * _cnormal(rng, S)
    iters = [0, 1, 3]
    labs, vs = sr.ld_cnc_receive(iters, rx, const, F, pa, sat, p, coeff, alpha)
    assert sorted(labs) == [0, 1, 2, 3]
    want_l = rm.cnc_receive([0, 1, 2, 3], rx, const, F, pa, sat, p, coeff, alpha)
    want_v = rm.cnc_receive([0, 1, 2, 3], rx, const, F, pa, sat, p, coeff, alpha, return_bits=False)
    for it in range(4):
        if sr.slicer_margin(vs[it], M) > 1e-9:
            np.testing.assert_array_equal(labs[it], want_l[it])
        l2, _ = pu.errors(want_v[it], vs[it])
        assert l2.max() <= 4 * np.log2(F) * U, (it, l2)
    assert np.array_equal(np.asarray(vs[0], complex), rx)


def test_slicer_margin():
    assert sr.slicer_margin([0.5 + 0.5j], 4) == 0.5
    assert sr.slicer_margin([1.0 + 100j], 4) == 1.0          # M = 4: the axes are the only boundaries
    assert sr.slicer_margin([2.25 + 1j, 1 - 3j], 16) == 0.25  # M = 16: -2, 0, 2
    assert sr.slicer_margin([5 + 5j], 16) == 3.0              # outside: the clamp has no boundary


def test_rel_err_handles_zero_references():
    e = sr.rel_err(np.array([0j, 1e-300, 2.0]), np.array([0j, 0j, 1.0]))
    assert e[0] == 0 and np.isinf(e[1]) and e[2] == 1.0
