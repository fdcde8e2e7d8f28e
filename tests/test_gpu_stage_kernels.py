"""The float64 stage kernels (csrc/stages.hip, the object API's fine seams) called directly
through _engine's helpers, at the sizes and values where such kernels go wrong: one element,
a partial wave, a partial block, and BIG = 2^20 + 257 elements -- one pass of the largest grid
(4096 blocks of 256 threads, grid_for) plus a full and a partial block of the second pass.

Index paths (QAM map / slice, bit counting, bin placement, the cyclic prefix, CNC labels) are
compared exactly with oracle/refmath.py.  Value paths are compared with the long-double
references of tests/stage_ref.py: a kernel may lose FACTOR = 16 (4 bits) against the error the
float64 oracle itself has against the same reference at the same input (the convention of
tests/test_gpu_probe_fft.py and test_stage_fft_against_long_double); the oracle's error is
measured here, never assumed, and must be > 0.  MRT and combine have first-order bounds of
their own, derived at the tests.  Every ratio is printed as a PROBE_SEAM line; the record of
an MI355X run is profiles/r10/stages/accuracy.md.

Large inputs tile a short pattern whose length is no multiple of the block, so the oracle and
the long-double reference run on the pattern only, and the kernel's output must repeat with
the pattern bit for bit."""
import functools

import numpy as np
import pytest

import probe_util as pu
import stage_ref as sr
from oracle import refmath as rm

pytestmark = pytest.mark.gpu

FACTOR = 16.0
U = sr.U
BIG = sr.BIG
SIZES = (1, 255, 256, 257, BIG)
ALL_M = (4, 16, 64, 256, 1024, 4096)


def _cnormal(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)


def _bits(a):
    """The array's float64 words as integers: equality of these is equality bit for bit."""
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def _tiled(pattern, n):
    return np.resize(pattern, n)


def _assert_repeats(got, period):
    """got[i] == got[i % period] bit for bit (the kernel is a function of the element alone)."""
    got = np.ascontiguousarray(got).reshape(-1)
    head = got[:period]
    assert np.array_equal(_bits(got) if got.dtype.kind in "fc" else got,
                          _bits(np.resize(head, got.size)) if got.dtype.kind in "fc" else np.resize(head, got.size))


def _report(seam, case, err, e_ref):
    print(f"PROBE_SEAM|{seam}|{case}|err={err:.3e}|oracle={e_ref:.3e}|ratio={err / e_ref:.2f}")


# ---------------------------------------------------------------- QAM map / slice (exact)
@pytest.mark.parametrize("M", ALL_M)
def test_qam_map_every_label(M):
    import _engine
    got = _engine.qam_map(M, np.arange(M))
    assert np.array_equal(_bits(got), _bits(rm.gray_qam_constellation(M)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("M", [16, 4096])
def test_qam_map_sizes(M, n):
    import _engine
    rng = np.random.default_rng(M + n)
    pattern = np.concatenate((rng.permutation(M), [M - 1, 0, M // 2]))[:4099]  # odd lengths 19 and 4099
    got = _engine.qam_map(M, _tiled(pattern, n))
    assert got.shape == (n,)
    assert np.array_equal(_bits(got), _bits(_tiled(rm.gray_qam_constellation(M)[pattern], n)))


@pytest.mark.parametrize("M", ALL_M)
def test_qam_slice_round_trip_ties_and_clamp(M):
    """Every label's own point; every even-integer lattice point of [-L-2, L+2]^2 (all two- and
    four-way ties of the constellation, and the ring outside it); points far outside, signed
    zeros and denormals -- against the brute-force argmin with its lowest-label tie-break.
    Then +-2^40 and +-1e300 on either axis, where the slicer's floor no longer fits its integer
    (and the brute force's squared distances overflow): the corner labels, written out by hand."""
    import _engine
    const = rm.gray_qam_constellation(M)
    L = int(np.sqrt(M))
    assert np.array_equal(_engine.qam_slice(M, const), np.arange(M))
    g = np.arange(-L - 2, L + 3, 2).astype(np.float64)
    lattice = (g[:, None] + 1j * g[None, :]).reshape(-1)
    assert np.array_equal(_engine.qam_slice(M, lattice), rm.detect_labels(const, lattice))
    tiny = np.nextafter(0.0, 1.0)
    ax = np.array([0.0, -0.0, tiny, -tiny, 1e-310, -1e-310, 0.5, -0.5, L - 1.0, 1.0 - L, L + 0.5, -L - 0.5,
                   1e3, -1e3, 1e6, -1e6, 999999.5, -999999.5])
    edge = (ax[:, None] + 1j * ax[None, :]).reshape(-1)
    assert np.array_equal(_engine.qam_slice(M, edge), rm.detect_labels(const, edge))
    # An axis label is the Gray code of the level's index: 0 for the lowest level 1 - L, and
    # gray(L - 1) = L / 2 for the highest, L - 1.  The label is (I's << hb) | Q's.
    hb, top = L.bit_length() - 1, L // 2
    for big in (2.0 ** 40, 1e300):
        far = np.array([big + 1j * big, big - 1j * big, -big + 1j * big, -big - 1j * big,
                        big + 1j * (1 - L), -big + 1j * (L - 1), (1 - L) + 1j * big, (L - 1) - 1j * big])
        want = [(top << hb) | top, top << hb, top, 0,
                top << hb, top, top, top << hb]
        assert np.array_equal(_engine.qam_slice(M, far), want), big


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("M", [16, 4096])
def test_qam_slice_sizes(M, n):
    import _engine
    L = int(np.sqrt(M))
    rng = np.random.default_rng(M + n)
    pattern = rng.uniform(-L - 1, L + 1, 509) + 1j * rng.uniform(-L - 1, L + 1, 509)
    pattern[::50] = np.round(pattern[::50].real / 2) * 2 + 1j * np.round(pattern[::50].imag / 2) * 2  # ties
    got = _engine.qam_slice(M, _tiled(pattern, n))
    assert got.shape == (n,)
    assert np.array_equal(got, _tiled(rm.detect_labels(rm.gray_qam_constellation(M), pattern), n))


# ---------------------------------------------------------------- bit counting (exact)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, BIG])
def test_count_bit_errors_sizes(n):
    import _engine
    rng = np.random.default_rng(n)
    a = rng.integers(0, 2, n)
    b = rng.integers(0, 2, n)
    assert _engine.count_bit_errors(a, b) == int(np.sum(a ^ b))
    assert _engine.count_bit_errors(a, a) == 0
    assert _engine.count_bit_errors(a, 1 - a) == n


# ---------------------------------------------------------------- OFDM
OFDM_GEOMETRIES = [(128, 4, 0), (128, 126, 128), (256, 6, 7), (2048, 1024, 128), (8192, 4096, 1)]


@pytest.mark.parametrize("F,S,cp", OFDM_GEOMETRIES)
def test_ofdm_tx_places_each_sub_carrier_in_its_bin(F, S, cp):
    """One-hot symbol vectors: the body's spectrum has the value in the bin rm.inband_bins
    names and nothing elsewhere.  Leakage bound (8 log2 F) u |v|: each of the F samples
    |v| / sqrt(F) carries a few u of relative error, which sum to at most that many u |v| in a
    bin, and the checking FFT adds u log2 F of its own; a misplaced bin is an error of |v|."""
    import _engine
    ks = list(range(S)) if S <= 126 else [0, 1, S // 2 - 1, S // 2, S // 2 + 1, S - 1]
    v = 0.75 - 1.25j
    sym = np.zeros((len(ks), S), complex)
    sym[np.arange(len(ks)), ks] = v
    td = _engine.ofdm_tx(sym, F, S, cp)
    assert td.shape == (len(ks), F + cp)
    spec = np.fft.fft(td[:, cp:], axis=-1, norm="ortho")
    bins = rm.inband_bins(F, S)[ks]
    want = np.zeros((len(ks), F), complex)
    want[np.arange(len(ks)), bins] = v
    assert np.all(np.argmax(np.abs(spec), axis=-1) == bins)
    assert np.max(np.abs(spec - want)) <= 8 * np.log2(F) * U * abs(v)
    assert np.array_equal(_bits(td[:, :cp]), _bits(td[:, F:]))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("F,S,cp", OFDM_GEOMETRIES)
def test_ofdm_tx_rx_against_long_double(F, S, cp, batch):
    import _engine
    rng = np.random.default_rng(F + S + cp + batch)
    sym = _cnormal(rng, (batch, S))
    tx_np = rm.ofdm_tx(sym, F, S, cp)
    rx_in = tx_np + 0.1 * _cnormal(rng, tx_np.shape)  # full band, and a prefix that is no copy
    cases = (("ofdm_tx", _engine.ofdm_tx(sym, F, S, cp), tx_np, sr.ld_ofdm_tx(sym, F, S, cp)),
             ("ofdm_rx", _engine.ofdm_rx(rx_in, F, S, cp), rm.ofdm_rx(rx_in, F, S, cp),
              sr.ld_ofdm_rx(rx_in, F, S, cp)))
    for seam, got, want, ref in cases:
        assert got.shape == want.shape
        e_np = [e.max() for e in pu.errors(want, ref)]  # the oracle's worst row
        assert e_np[0] > 0 and e_np[1] > 0
        l2, mx = (e.max() for e in pu.errors(got, ref))
        _report(seam, f"F={F}|S={S}|cp={cp}|batch={batch}|l2", l2, e_np[0])
        _report(seam, f"F={F}|S={S}|cp={cp}|batch={batch}|mx", mx, e_np[1])
        assert l2 <= FACTOR * e_np[0]
        assert mx <= FACTOR * e_np[1]
        if seam == "ofdm_tx":  # the prefix is the body's tail
            assert np.array_equal(_bits(got[:, :cp]), _bits(got[:, F:]))


def test_ofdm_batch_beyond_one_grid_pass():
    """F 128, cp 0, 8193 symbols: 2^20 + 128 samples, so the bin-mapping and prefix kernels take
    a second grid pass (row 8192 starts at element 2^20).  The rows repeat a 7-row pattern, so
    every row must equal its pattern row's result bit for bit; the first and last rows and the
    rows around element 2^20 are compared with long double."""
    import _engine
    F, S, cp, batch, period = 128, 126, 0, 8193, 7
    assert batch * F > sr.GRID_PASS
    rng = np.random.default_rng(8193)
    pat = _cnormal(rng, (period, S))
    sym = pat[np.arange(batch) % period]
    rows = np.array([0, 1, 8190, 8191, 8192])
    td = _engine.ofdm_tx(sym, F, S, cp)
    assert td.shape == (batch, F)
    assert np.array_equal(_bits(td), _bits(td[:period][np.arange(batch) % period]))
    rx_pat = rm.ofdm_tx(pat, F, S, cp) + 0.1 * _cnormal(rng, (period, F))
    rx_in = rx_pat[np.arange(batch) % period]
    back = _engine.ofdm_rx(rx_in, F, S, cp)
    assert back.shape == (batch, S)
    assert np.array_equal(_bits(back), _bits(back[:period][np.arange(batch) % period]))
    for seam, got, want, ref in (("ofdm_tx", td[rows], rm.ofdm_tx(sym[rows], F, S, cp), sr.ld_ofdm_tx(sym[rows], F, S, cp)),
                                 ("ofdm_rx", back[rows], rm.ofdm_rx(rx_in[rows], F, S, cp),
                                  sr.ld_ofdm_rx(rx_in[rows], F, S, cp))):
        e_np = [e.max() for e in pu.errors(want, ref)]
        assert e_np[0] > 0 and e_np[1] > 0
        l2, mx = (e.max() for e in pu.errors(got, ref))
        _report(seam, f"F={F}|S={S}|cp={cp}|batch={batch}|l2", l2, e_np[0])
        _report(seam, f"F={F}|S={S}|cp={cp}|batch={batch}|mx", mx, e_np[1])
        assert l2 <= FACTOR * e_np[0]
        assert mx <= FACTOR * e_np[1]


# ---------------------------------------------------------------- PA
PA_SAT = 2.25  # sqrt(sat) = 1.5: |x|^2 = sat exactly on the axes
PA_TOI = 0.05 / PA_SAT
PA_CASES = [("none", 0.0), ("softlim", 0.0), ("toi", 0.0)] + [("rapp", p) for p in (0.5, 2.0, 2.5, 3.0, 10.0)]


@functools.lru_cache(maxsize=None)
def _pa_pattern():
    """263 values: a clipped sample first (the n = 1 case), zeros of both signs, |x|^2 = sat
    exactly and one float either side on both axes, 1e-160, and amplitudes 1e-3 ... 1e3 sqrt(sat)
    at random phases."""
    rng = np.random.default_rng(77)
    r = 1.5
    edge = [r, np.nextafter(r, 0), np.nextafter(r, 2)]
    special = [3.0 * np.exp(0.7j), 0j, complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)]
    special += [complex(s * e, 0) for e in edge for s in (1, -1)] + [complex(0, s * e) for e in edge for s in (1, -1)]
    special += [1e-160, 1e-160j, complex(1e-160, -1e-160)]
    amp = np.geomspace(1e-3, 1e3, 263 - len(special)) * r
    x = np.concatenate((special, amp * np.exp(2j * np.pi * rng.uniform(size=amp.size))))
    assert x.size == 263
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("n", [1, 257, BIG])
@pytest.mark.parametrize("kind,p", PA_CASES)
def test_pa_against_long_double(kind, p, n):
    """Per element |got - ref| / |ref| (equality where ref = 0); the worst element of the kernel
    against the worst element of the oracle.  MIMO_PA_NONE is the identity, bit for bit."""
    import _engine
    pattern = _pa_pattern()
    x = _tiled(pattern, n)
    got = _engine.pa(kind, x, PA_SAT, p, PA_TOI)
    assert got.shape == (n,)
    if n > pattern.size:
        _assert_repeats(got, pattern.size)
    m = min(n, pattern.size)
    got, x = got[:m], x[:m]
    if kind == "none":
        assert np.array_equal(_bits(got), _bits(x))
        return
    ref = pu.ld_pa(sr.PA_CODE[kind], x, PA_SAT, p, PA_TOI)
    with np.errstate(all="ignore"):  # the oracle's soft limiter forms sat / |x|^2 for 1e-160 too, and discards it
        e_np = sr.rel_err(rm.apply_pa(kind, x, PA_SAT, p, PA_TOI), ref).max()
        if n == 1:
            # one sample: the oracle's error there may be small by luck; its error over the pattern stands in
            e_np = sr.rel_err(rm.apply_pa(kind, pattern, PA_SAT, p, PA_TOI),
                              pu.ld_pa(sr.PA_CODE[kind], pattern, PA_SAT, p, PA_TOI)).max()
    assert 0 < e_np < np.inf
    err = sr.rel_err(got, ref).max()
    _report("pa", f"kind={kind}|p={p}|n={n}", err, e_np)
    assert err <= FACTOR * e_np


# ---------------------------------------------------------------- LLR
LLR_VAR_FLOOR = {4: 0.3, 16: 0.3, 64: 0.3, 256: 2.0}  # M = 256: 24^2 2 / 0.3 would underflow every far term


@pytest.mark.parametrize("M", [4, 16, 64, 256])
def test_qam_llr_against_long_double(M):
    """257 points over [-L-1, L+1]^2, each with its own noise variance, chosen so that every LLR
    of the oracle is finite.  Metric |got - ref| / max(1, |ref|), worst entry."""
    import _engine
    L = int(np.sqrt(M))
    rng = np.random.default_rng(M)
    z = rng.uniform(-L - 1, L + 1, 257) + 1j * rng.uniform(-L - 1, L + 1, 257)
    nv = rng.uniform(LLR_VAR_FLOOR[M], 8.0, 257)
    const = rm.gray_qam_constellation(M)
    want = rm.soft_llr(const, z, nv).reshape(257, -1)
    assert np.all(np.isfinite(want))
    ref = sr.ld_llr(const, z, nv)
    scale = np.maximum(1, np.abs(ref))
    e_np = float(np.max(np.abs(want - ref) / scale))
    assert e_np > 0
    got = _engine.qam_llr(M, z, nv).reshape(257, -1)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = float(np.max(np.abs(got - ref) / scale))
    _report("qam_llr", f"M={M}|n=257", err, e_np)
    assert err <= FACTOR * e_np


@pytest.mark.parametrize("M", [4, 16, 64, 256])
def test_qam_llr_infinities(M):
    """Noise variance 1e-3 at points within 0.1 (per axis) of a constellation point, and
    0.9 + 1.1j: every exponent -|z - C|^2 / nv is above -600 or below -900 (checked here), far
    on either side of exp's underflow at -745, so which sums are zero does not depend on
    rounding.  Every LLR is then +inf (zero-bit sum 0) or -inf (one-bit sum 0), and the
    pattern must be the oracle's."""
    import _engine
    const = rm.gray_qam_constellation(M)
    rng = np.random.default_rng(M + 1)
    z = np.concatenate((const[rng.integers(0, M, 256)] + rng.uniform(-0.1, 0.1, 256)
                        + 1j * rng.uniform(-0.1, 0.1, 256), [0.9 + 1.1j]))
    e = sr.llr_exponents(const, z, 1e-3)
    assert np.all((e > -600) | (e < -900))
    want = rm.soft_llr(const, z, 1e-3)
    assert np.all(np.isinf(want)) and np.any(want > 0) and np.any(want < 0)
    got = _engine.qam_llr(M, z, 1e-3)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- AWGN
AWGN_KEYS = [(1, 0), (0x0123456789ABCDEF, 7), (2 ** 63 - 1, 2 ** 32 + 5)]
AWGN_STD = 0.37


def _awgn_probe_indices(n):
    """Where the long-double values are formed: everything up to 512, everything from 512 before
    the end of the first grid pass on, and every 997th element between."""
    if n <= 2048:
        return np.arange(n)
    return np.unique(np.concatenate((np.arange(512), np.arange(sr.GRID_PASS - 512, n), np.arange(0, n, 997))))


@pytest.mark.parametrize("n", [1, 257, BIG])
@pytest.mark.parametrize("seed,counter", AWGN_KEYS)
def test_awgn_values(seed, counter, n):
    """out = in + n_i with n_i the Philox / Box-Muller value of element i.  Error relative to
    |n_i|; the yardstick is the float64 NumPy formula (oracle.philox.box_muller) added to the
    same input.  The input is non-zero but small (1e-6), so that the rounding of the sum, which
    kernel and oracle share, does not drown the noise value's own error -- a result without
    the input, or with its parts swapped, is still off by 1e-6 / |n_i|, nine orders above the
    bound."""
    import _engine
    rng = np.random.default_rng(n)
    x = _tiled(1e-6 * _cnormal(rng, 1009), n)
    got = _engine.awgn(x, AWGN_STD, seed, counter)
    assert got.shape == (n,)
    idx = _awgn_probe_indices(n)
    noise = sr.ld_awgn_noise(seed, counter, idx, AWGN_STD)
    ref = x[idx].astype(sr.CLD) + noise
    mod = np.abs(noise)
    # the oracle's error over the same elements; for n = 1 over the first 257 (one sample's may be small by luck)
    j = idx if n > 1 else np.arange(257)
    xj = x[idx] if n > 1 else _tiled(x, 257)
    nj = noise if n > 1 else sr.ld_awgn_noise(seed, counter, j, AWGN_STD)
    e_np = float(np.max(np.abs((xj + sr.np_awgn_noise(seed, counter, j, AWGN_STD)) - (xj.astype(sr.CLD) + nj))
                        / np.abs(nj)))
    assert e_np > 0
    err = float(np.max(np.abs(got[idx] - ref) / mod))
    _report("awgn", f"seed={seed:#x}|counter={counter}|n={n}", err, e_np)
    assert err <= FACTOR * e_np
    if n > 2048:  # every element, coarsely: the float64 formula is within 1e-12 of each value
        full = x + sr.np_awgn_noise(seed, counter, np.arange(n), AWGN_STD)
        assert np.max(np.abs(got - full)) <= 1e-12


def test_awgn_high_words_of_counter_and_seed_matter():
    import _engine
    x = np.zeros(257, complex)
    lo = _engine.awgn(x, AWGN_STD, 2 ** 63 - 1, 5)
    hi = _engine.awgn(x, AWGN_STD, 2 ** 63 - 1, 2 ** 32 + 5)
    assert not np.any(lo == hi)
    s0 = _engine.awgn(x, AWGN_STD, 0x89ABCDEF, 7)
    s1 = _engine.awgn(x, AWGN_STD, 0x0123456789ABCDEF, 7)
    assert not np.any(s0 == s1)
    assert np.array_equal(_bits(lo), _bits(_engine.awgn(x, AWGN_STD, 2 ** 63 - 1, 5)))  # and the same call repeats


# ---------------------------------------------------------------- CNC
CNC_CASES = [(128, 4, 4, "softlim", 0.0), (256, 252, 64, "rapp", 2.5), (2048, 1024, 256, "toi", 0.0),
             (8192, 4096, 16, "softlim", 0.0)]
CNC_LISTS = [[0, 1, 3, 7], [2], [0]]
CNC_LAST = 7
CNC_MARGIN = 1e-6


@functools.lru_cache(maxsize=None)
def _cnc_case(F, S, M, pa, p):
    """A received in-band vector (random symbols through the PA chain, scaled by 1 / alpha, plus
    noise), the PA parameters, and the float64 oracle's and the long-double loop's labels and
    slicer inputs of every iteration 0 ... 7.  The condition under which labels must agree
    exactly and values to rounding is asserted here with nothing left out: at every iteration
    the two loops decide alike and no slicer input is within 1e-6 of a decision boundary."""
    const = rm.gray_qam_constellation(M)
    rng = np.random.default_rng(F + S + M)
    avg = rm.ofdm_avg_sample_power(const, F, S)
    # a hard-driven PA (IBO -2 dB, third-order intercept 8 dB) and strong noise: the loop is still
    # changing labels at iteration 7, so every listed iteration has a row of its own
    sat, coeff = rm.sat_pow(-2.0, avg), rm.toi_coeff(8.0, avg)
    alpha = float(rm.calc_alpha(-2.0)) if pa == "softlim" else 0.9
    bins = rm.inband_bins(F, S)
    up = np.zeros(F, complex)
    up[bins] = const[rng.integers(0, M, S)]
    rx = np.fft.fft(rm.apply_pa(pa, np.fft.ifft(up, norm="ortho"), sat, p, coeff), norm="ortho")[bins] / alpha
    rx = rx + 0.5 * _cnormal(rng, S)
    every = list(range(CNC_LAST + 1))
    labs_np = rm.cnc_receive(every, rx, const, F, pa, sat, p, coeff, alpha)
    vs_np = rm.cnc_receive(every, rx, const, F, pa, sat, p, coeff, alpha, return_bits=False)
    labs_ld, vs_ld = sr.ld_cnc_receive(every, rx, const, F, pa, sat, p, coeff, alpha)
    for it in every:
        assert np.array_equal(labs_ld[it], labs_np[it]), it
        assert sr.slicer_margin(vs_ld[it], M) >= CNC_MARGIN, it
        assert sr.slicer_margin(vs_np[it], M) >= CNC_MARGIN, it
    if S > 4:  # (four carriers settle at once) a row of another iteration would be noticed
        rows = [0, 1, 2, 3, 7]
        assert all(np.any(labs_np[a] != labs_np[b]) for i, a in enumerate(rows) for b in rows[i + 1:])
    return rx, sat, coeff, alpha, labs_np, vs_np, vs_ld


@pytest.mark.parametrize("iters", CNC_LISTS, ids=lambda v: "it" + "_".join(map(str, v)))
@pytest.mark.parametrize("F,S,M,pa,p", CNC_CASES)
def test_cnc_receive_labels_and_corrected_symbols(F, S, M, pa, p, iters):
    """Lists with gaps, without iteration 0 and of iteration 0 alone: row j of the output is the
    j-th listed iteration.  Labels equal the oracle's; the corrected symbols rx - d stay within
    16 x the oracle's error (its worst listed iteration) of the long-double loop.  Iteration 0
    is the input itself, bit for bit."""
    import _engine
    rx, sat, coeff, alpha, labs_np, vs_np, vs_ld = _cnc_case(F, S, M, pa, p)
    got = _engine.cnc_receive(M, F, pa, sat, p, coeff, alpha, iters, rx)
    assert sorted(got) == iters
    for it in iters:
        assert np.array_equal(got[it], labs_np[it]), it
    cor = _engine.cnc_receive(M, F, pa, sat, p, coeff, alpha, iters, rx, return_bits=False)
    assert sorted(cor) == iters
    later = [it for it in iters if it > 0]
    if 0 in iters:
        assert np.array_equal(_bits(cor[0]), _bits(rx))
    if not later:
        return
    e_np = np.max([pu.errors(vs_np[it], vs_ld[it]) for it in later], axis=0)
    assert e_np[0] > 0 and e_np[1] > 0
    for it in later:
        l2, mx = pu.errors(cor[it], vs_ld[it])
        _report("cnc_receive", f"F={F}|S={S}|M={M}|pa={pa}|iters={iters}|it={it}|l2", float(l2), float(e_np[0]))
        _report("cnc_receive", f"F={F}|S={S}|M={M}|pa={pa}|iters={iters}|it={it}|mx", float(mx), float(e_np[1]))
        assert l2 <= FACTOR * e_np[0]
        assert mx <= FACTOR * e_np[1]


# ---------------------------------------------------------------- MRT / combine (derived bounds)
MRT_SHAPES = [(1, 1), (1, 257), (3, 5), (64, 300), (4096, 4)]
HIGHER_ORDER = 1.01  # the bounds are first order in u


def _channel(rng, A, K):
    """Per-antenna magnitudes 1e-3 ... 1e3."""
    return _cnormal(rng, (A, K)) * 10.0 ** rng.uniform(-3, 3, (A, 1))


@pytest.mark.parametrize("A,K", MRT_SHAPES)
def test_mrt_precode_within_its_rounding_bound(A, K):
    """|p - ref| <= (A / 2 + 4) u |ref|: each |h|^2 = re^2 + im^2 carries 2 u, summing A
    non-negative terms one after the other adds at most (A - 1) u, the square root halves the
    (A + 1) u and adds u (correctly rounded), the divide and the product add u each:
    (A + 1) / 2 + 3 <= A / 2 + 4."""
    import _engine
    h = _channel(np.random.default_rng(1000 * A + K), A, K)
    ref = sr.ld_mrt(h)
    got = _engine.mrt_precode(h)
    assert got.shape == (A, K)
    ratio = np.asarray(np.abs(got - ref) / (U * np.abs(ref)), np.float64)
    print(f"PROBE_SEAM|mrt_precode|A={A}|K={K}|err_u={ratio.max():.2f}|bound_u={A / 2 + 4:.1f}")
    assert np.all(ratio <= (A / 2 + 4) * HIGHER_ORDER)


def _assert_combine(case, h, y, got):
    """|out - ref| <= sqrt(2) (A + 2) u sum_a |h_a| |y_a| per column: a complex product's
    parts are each within 2 u |h||y| of exact (two products, one sum), sequential summation of
    A terms adds (A - 1) u of the running sums, each at most sum |h||y|: (A + 1) u per part,
    rounded up to A + 2, and sqrt(2) for the two parts."""
    A = h.shape[0]
    ref, scale = sr.ld_combine(h, y)
    ratio = np.asarray(np.abs(got - ref) / (U * scale), np.float64)
    print(f"PROBE_SEAM|combine|{case}|err_u={ratio.max():.3f}|bound_u={np.sqrt(2) * (A + 2):.1f}")
    assert np.all(ratio <= np.sqrt(2) * (A + 2) * HIGHER_ORDER)


@pytest.mark.parametrize("A,K", MRT_SHAPES)
def test_combine_within_its_rounding_bound(A, K):
    import _engine
    rng = np.random.default_rng(2000 * A + K)
    h, y = _channel(rng, A, K), _cnormal(rng, (A, K))
    got = _engine.combine(h, y)
    assert got.shape == (K,)
    _assert_combine(f"A={A}|K={K}", h, y, got)


def test_combine_sum_that_cancels():
    """The last antenna's signal is set so that sum h y is about 1e-12 of sum |h||y| (asserted):
    the error bound does not shrink with the result, and a result-relative tolerance would
    have been the wrong yardstick."""
    import _engine
    A, K = 64, 300
    rng = np.random.default_rng(64300)
    h, y = _channel(rng, A, K), _cnormal(rng, (A, K))
    partial = np.sum(h[:-1] * y[:-1], axis=0)
    scale = np.sum(np.abs(h[:-1]) * np.abs(y[:-1]), axis=0) + np.abs(partial)
    y[-1] = -(partial / h[-1]) * (1 - 1e-12 * scale / np.abs(partial))
    ref, sc = sr.ld_combine(h, y)
    frac = np.asarray(np.abs(ref) / sc, np.float64)
    assert np.all((frac > 1e-13) & (frac < 1e-11))
    _assert_combine(f"A={A}|K={K}|cancelling", h, y, _engine.combine(h, y))


def test_combine_columns_beyond_one_grid_pass():
    import _engine
    A, period = 8, 251
    rng = np.random.default_rng(8251)
    hp, yp = _channel(rng, A, period), _cnormal(rng, (A, period))
    col = np.arange(BIG) % period
    got = _engine.combine(hp[:, col], yp[:, col])
    assert got.shape == (BIG,)
    _assert_repeats(got, period)
    _assert_combine(f"A={A}|K={BIG}", hp, yp, got[:period])
