"""Soft mode on a machine without a GPU: the width helper, the host-side argument checks of
mimo_engine_soft_points (no HIP call before them), SoftStats arithmetic on hand-made histograms, the
binned GMI against the unbinned one, the reference metric (tests/soft_ref.py) against the oracle's
exact LLR, and sweep.gmi_vs_ebn0 with its CSV writer against a fake link."""
import ctypes
import math
import shutil
import subprocess

import numpy as np
import pytest

import _engine
import fake_soft_link as fsl
import soft_ref
from oracle import refmath as rm


def _engine_handle(precision=0):
    lib = _engine.lib()
    tx = np.zeros((4, 3))
    fr = np.full(512, 3.5e9)
    dp = ctypes.POINTER(ctypes.c_double)
    c = _engine.MimoConfig(n_ant=4, n_sub_carr=256, n_fft=512, constel_size=16, cp_len=16, channel_kind=1,
                           receiver_kind=1, device=-1, rx_loc_var=10.0, reroll_chan=1, precision=precision,
                           tx_pos=tx.ctypes.data_as(dp), carrier_freqs=fr.ctypes.data_as(dp))
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h
    return lib, h, (tx, fr)


def _soft(lib, h, iters, out, rho_max=16.0, n_trials=8):
    pt = _engine.Engine.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9)
    it = np.asarray(iters, np.int32)
    one = lambda v: np.asarray([v], np.uint64)  # noqa: E731
    seeds, first, n = one(1), one(0), one(n_trials)
    err = np.zeros(40, np.uint64)
    bits = np.zeros(40, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_soft_points(h, 1, ctypes.byref(pt), seeds.ctypes.data_as(u64), first.ctypes.data_as(u64),
                                     n.ctypes.data_as(u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     len(it), 0, err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None,
                                     ctypes.c_double(rho_max),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if out is not None else None,
                                     None)
    return rc, lib.mimo_last_error().decode()


# ---------------------------------------------------------------- width
def test_soft_width():
    lib = _engine.lib()
    assert _engine.SOFT_BINS == 256 == soft_ref.SOFT_BINS
    assert lib.mimo_soft_width(1, 0) == 256 and lib.mimo_soft_width(3, 1) == 1024
    assert lib.mimo_soft_width(32, 1) == 8448
    for bad in (0, -1, 33):
        assert lib.mimo_soft_width(bad, 0) == -1 and "n_iters" in lib.mimo_last_error().decode()


# ---------------------------------------------------------------- validation, before any HIP call
def test_soft_rejects_float32_engine_before_any_hip_call():
    lib, h, keep = _engine_handle(precision=1)
    out = np.full(256, 7.0)
    rc, msg = _soft(lib, h, [0], out)
    assert rc == -1 and "float64" in msg and "soft" in msg, (rc, msg)
    assert np.all(out == 7.0)  # nothing added
    lib.mimo_engine_destroy(h)


def test_soft_rejects_null_soft_out_before_any_hip_call():
    lib, h, keep = _engine_handle()
    rc, msg = _soft(lib, h, [0], None)
    assert rc == -1 and "soft_out" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("rho_max", [0.0, -1.0, float("nan"), float("inf"), float("-inf"), 1e-320])
def test_soft_rejects_bad_rho_max_before_any_hip_call(rho_max):
    """Not finite, not > 0, or (a subnormal) with an infinite scale 128 / rho_max: MIMO_EINVAL with a
    message that names rho_max."""
    lib, h, keep = _engine_handle()
    out = np.full(256, 7.0)
    rc, msg = _soft(lib, h, [0], out, rho_max)
    assert rc == -1 and "rho_max" in msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("iters", [[2, 1], [], list(range(33))])
def test_soft_rejects_bad_iters_before_any_hip_call(iters):
    lib, h, keep = _engine_handle()
    out = np.full(256 * 34, 7.0)
    rc, msg = _soft(lib, h, iters, out)
    assert rc == -1 and msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


def test_abi8_library_without_soft_is_reported_by_name(tmp_path, monkeypatch):
    """The soft entry points were added within ABI 8: a library that answers 8 and exports everything
    but them is reported as lacking a named entry point ('rebuild it')."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    mine = ("mimo_soft_width", "mimo_engine_soft_points", "mimo_qam_softbits")
    assert all(n in _engine.SYMBOLS for n in mine)
    names = [n for n in _engine.SYMBOLS if n not in mine]
    src = tmp_path / "stale.c"
    src.write_text("int mimo_abi_version(void) { return 8; }\n" +
                   "".join(f"void {n}(void) {{}}\n" for n in names if n != "mimo_abi_version"))
    so = tmp_path / "libstale8.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(so))
    with pytest.raises(_engine.EngineError, match=r"\(ABI 8\) lacks mimo_soft_width: rebuild it"):
        _engine.lib()


# ---------------------------------------------------------------- SoftStats on hand-made histograms
def hand_hist():
    """rho_max 128: bins one unit wide, centres b - 127.5.  Index 0: one reliability at -0.5, three at
    +1.5.  Index 1: one in each end bin, two at +0.5."""
    h = np.zeros((2, 256))
    h[0, 127], h[0, 129] = 1, 3
    h[1, 0], h[1, 255], h[1, 128] = 1, 1, 2
    return h


def f2(x):
    return math.log2(1.0 + math.exp(-x))


def test_soft_stats_exact_values():
    st = _engine.SoftStats(hand_hist(), 128.0, 16, 1)
    assert (st.n_idx, st.rho_max, st.constel_size, st.n_trials, st.width) == (2, 128.0, 16, 1, 1.0)
    np.testing.assert_array_equal(st.centres, np.arange(256) - 127.5)
    np.testing.assert_array_equal(st.n_bits, [4, 4])
    np.testing.assert_array_equal(st.ber(), [0.25, 0.25])
    np.testing.assert_array_equal(st.clamped(), [0.0, 0.5])
    assert st.nominal_scale(0.5) == 8.0
    for s in (0.25, 1.0, 3.0):
        want = [1 - (f2(-0.5 * s) + 3 * f2(1.5 * s)) / 4, 1 - (f2(-127.5 * s) + f2(127.5 * s) + 2 * f2(0.5 * s)) / 4]
        np.testing.assert_allclose(st.gmi(s), want, rtol=1e-14, atol=1e-15)
    # one scale per index
    np.testing.assert_array_equal(st.gmi([0.25, 3.0]), [st.gmi(0.25)[0], st.gmi(3.0)[1]])
    # index 0's best scale: where d/ds [f2(-s / 2) + 3 f2(3 s / 2)] = 0, i.e. sigma(s / 2) / 2 = 4.5 sigma(-3 s / 2)
    s0 = st.best_scale()[0]
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))  # noqa: E731
    assert abs(0.5 * sig(0.5 * s0) - 4.5 * sig(-1.5 * s0)) < 1e-6
    np.testing.assert_array_equal(st.gmi(), st.gmi(st.best_scale()))
    assert np.all(st.gmi() >= st.gmi(1.0)) and np.all(st.gmi() <= 1.0)
    np.testing.assert_array_equal(st.rate(), 4 * st.gmi())
    with pytest.raises(ValueError, match="rho_max"):
        _engine.SoftStats(hand_hist(), 0.0, 16, 1)
    with pytest.raises(ValueError):
        _engine.SoftStats(np.ones(255), 1.0, 16, 1)


def test_soft_stats_without_errors_saturates():
    """No cell below bin 128: the GMI grows with the scale towards 1 and the search ends at its upper end."""
    h = np.zeros((1, 256))
    h[0, 140] = 10
    st = _engine.SoftStats(h, 16.0, 4, 1)
    assert st.ber()[0] == 0.0 and st.gmi()[0] == pytest.approx(1.0, abs=1e-12)
    assert st.best_scale()[0] == pytest.approx(2e3 / st.width, rel=1e-6)


def test_soft_stats_pooling_and_empty():
    a = _engine.SoftStats(hand_hist(), 128.0, 16, 1)
    b = _engine.SoftStats(2 * hand_hist(), 128.0, 16, 2)
    for pooled in (a + b, a.pool(b)):
        np.testing.assert_array_equal(pooled.hist, 3 * hand_hist())
        assert pooled.n_trials == 3
        np.testing.assert_array_equal(pooled.ber(), a.ber())
        np.testing.assert_allclose(pooled.gmi(0.7), a.gmi(0.7), rtol=1e-15)
    with pytest.raises(ValueError, match="cannot be pooled"):
        a + _engine.SoftStats(hand_hist(), 64.0, 16, 1)
    with pytest.raises(ValueError, match="cannot be pooled"):
        a + _engine.SoftStats(hand_hist(), 128.0, 64, 1)
    with pytest.raises(ValueError, match="cannot be pooled"):
        a + _engine.SoftStats(hand_hist()[:1], 128.0, 16, 1)
    empty = _engine.SoftStats(np.zeros((2, 256)), 128.0, 16, 0)
    np.testing.assert_array_equal(empty.n_bits, [0, 0])
    np.testing.assert_array_equal(empty.ber(), [0, 0])
    np.testing.assert_array_equal(empty.clamped(), [0, 0])
    np.testing.assert_array_equal(empty.gmi(1.0), [0, 0])
    np.testing.assert_array_equal(empty.gmi(), [0, 0])
    np.testing.assert_array_equal((empty + a).hist, a.hist)


# ---------------------------------------------------------------- the binned GMI against the unbinned one
RHO_MAX_G = 8.0


def gaussian_stats():
    rho = np.random.default_rng(20261020).normal(2.0, 1.5, 200000)
    hist = np.bincount(soft_ref.bin_of(rho, RHO_MAX_G), minlength=256).astype(np.float64)
    return rho, _engine.SoftStats(hist, RHO_MAX_G, 16, 1)


@pytest.mark.parametrize("s", [0.25, 0.5, 1.0, 2.0, 4.0])
def test_gmi_against_the_unbinned_truth(s):
    """|gmi(s) - (1 - mean log2(1 + exp(-s rho)))| <= 0.045 (s w)^2 + clamped share x the largest
    per-sample term: replacing rho by its bin's midpoint moves s rho by at most s w / 2, and
    f(x) = log2(1 + exp(-x)) has f'' <= 1 / (4 ln 2), so the second-order term is at most
    f''_max (s w)^2 / 8 = 0.045 (s w)^2; a clamped sample is off by at most the larger of its own
    term and its end bin's."""
    rho, st = gaussian_stats()
    w = st.width
    assert w == RHO_MAX_G / 128
    truth = 1.0 - np.mean(np.logaddexp(0.0, -s * rho)) / math.log(2.0)
    largest = max(np.logaddexp(0.0, -s * rho).max(), np.logaddexp(0.0, -s * st.centres[0])) / math.log(2.0)
    bound = 0.045 * (s * w) ** 2 + st.clamped()[0] * largest
    dev = abs(st.gmi(s)[0] - truth)
    print(f"SOFT_GMI_BINNING s={s} dev={dev:.3e} bound={bound:.3e} clamped={st.clamped()[0]:.2e}")
    assert dev <= bound, (dev, bound)


def test_gmi_maximum_dominates_nominal_and_is_concave():
    rho, st = gaussian_stats()
    # rho = 2 + 1.5 n: an LLR scale * rho is consistent at scale = 2 mean / var
    nominal = 2 * 2.0 / 1.5 ** 2
    assert st.gmi()[0] >= st.gmi(nominal)[0]
    assert st.best_scale()[0] == pytest.approx(nominal, rel=0.05)
    grid = np.linspace(0.05, 8.0, 160)
    g = np.array([st.gmi(s)[0] for s in grid])
    assert np.all(np.diff(g, 2) <= 1e-13)       # concave in the scale
    assert np.all(g <= st.gmi()[0] + 1e-15)     # and nowhere above the maximum found


# ---------------------------------------------------------------- the metric against the exact LLR
@pytest.mark.parametrize("M", [4, 16, 64, 256])
def test_reference_metric_against_exact_llr(M):
    """|soft_llr - 4 lambda / noise_var| <= ln(M / 2): each of the exact LLR's two log-sums over M / 2
    points exceeds its largest term's logarithm by at most ln(M / 2)."""
    L = int(round(math.sqrt(M)))
    rng = np.random.default_rng(M)
    z = rng.uniform(-L - 1, L + 1, 500) + 1j * rng.uniform(-L - 1, L + 1, 500)
    const = rm.gray_qam_constellation(M)
    for nv in (2.0, 5.0):
        exact = rm.soft_llr(const, z, nv).reshape(len(z), -1)
        maxlog = 4.0 * soft_ref.lam(M, z) / nv
        assert np.all(np.isfinite(exact))
        dev = np.abs(exact - maxlog)
        print(f"SOFT_MAXLOG M={M} nv={nv} worst={dev.max():.4f} bound={math.log(M / 2):.4f}")
        assert np.all(dev <= math.log(M / 2))
    # the sign convention and the hard decision: lambda > 0 where the nearest point's bit is 1
    lab = rm.detect_labels(const, z)
    la = soft_ref.lam(M, z)
    np.testing.assert_array_equal(la[la != 0] > 0, soft_ref.label_bits(M, lab)[la != 0])
    r = soft_ref.rho(M, z, lab)
    assert np.all(r >= 0)


def test_reference_metric_by_hand():
    """16-QAM, levels -3 -1 1 3 with Gray codes 00 01 11 10.  x = 0.5: MSB d0 = 1.5, d1 = 0.5 ->
    lambda = 1 * 2 / 4 = 0.5; LSB d0 = min(3.5, 2.5) = 2.5, d1 = 0.5 -> 2 * 3 / 4 = 1.5.  x = -4:
    MSB d0 = 1, d1 = 5 -> -4 * 6 / 4 = -6; LSB d0 = 1, d1 = 3 -> -2 * 4 / 4 = -2."""
    np.testing.assert_array_equal(soft_ref.axis_lambda(16, [0.5, -4.0]), [[0.5, 1.5], [-6.0, -2.0]])
    np.testing.assert_array_equal(soft_ref.lam(16, [0.5 - 4.0j]), [[0.5, 1.5, -6.0, -2.0]])
    # bins: rho_max 16, width 1/8
    np.testing.assert_array_equal(soft_ref.bin_of([0.0, -1e-300, 0.125, -0.125, 15.99, 16.0, 1e9, -16.0, -16.01, -1e9],
                                                  16.0), [128, 127, 129, 127, 255, 255, 255, 0, 0, 0])


def test_doubling_rho_max_halves_the_bin_offsets():
    """rho_max doubled halves the scale exactly, so bin b moves to 128 + floor((b - 128) / 2) (for the
    reliabilities inside the narrower range; the end bins hide what lies beyond)."""
    rho = np.random.default_rng(5).normal(0.0, 4.0, 20000)
    rho = rho[np.abs(rho) < 16.0]
    b1, b2 = soft_ref.bin_of(rho, 16.0), soft_ref.bin_of(rho, 32.0)
    assert b1.min() >= 0 and b1.max() <= 255 and len(np.unique(b1)) > 200
    np.testing.assert_array_equal(b2, 128 + np.floor((b1 - 128) / 2).astype(np.int64))


# ---------------------------------------------------------------- sweep against the fake link
def test_gmi_vs_ebn0_and_csv_writer(tmp_path):
    import sweep
    from utilities import ebn0_to_snr, read_from_csv, save_to_csv
    link = fsl.FakeSoftLink()
    ibos, ebn0 = np.array([0.0, 4.0]), np.array([6.0, 10.0, 14.0])
    stats = sweep.gmi_vs_ebn0(link, ibos, ebn0, [0, 1], 5, seed=11)
    snr = [float(v) for v in ebn0_to_snr(ebn0, fsl.N_SC, fsl.N_SC, fsl.M)]
    assert len(link.calls) == 3  # the IBOs of one Eb/N0 in one call
    for j, call in enumerate(link.calls):
        assert call["ibos"] == [0.0, 4.0] and call["snrs"] == [snr[j]] * 2 and call["n_trials"] == 5
        assert call["iters"] == [0, 1] and call["incl_clean"] is False and call["reroll_chan"] is True
        assert call["rho_max"] is None
        assert call["seeds"] == [sweep.point_seed(11, i * 3 + j) for i in range(2)]
    assert len(stats) == 2 and all(len(r) == 3 for r in stats)
    for i, ibo in enumerate(ibos):
        for j in range(3):
            np.testing.assert_array_equal(stats[i][j].hist, fsl.fake_hist(ibo, snr[j], 5))
    sweep.gmi_vs_ebn0(link, ibos[:1], ebn0[:1], [0], 2, seed=11, incl_clean=True, reroll_chan=False, rho_max=4.0)
    assert link.calls[3]["rho_max"] == 4.0 and link.calls[3]["incl_clean"] is True
    assert link.calls[3]["reroll_chan"] is False
    rows = sweep.gmi_vs_ebn0_rows(ebn0, stats[1])
    save_to_csv(rows, "gmi", directory=str(tmp_path))
    back = np.asarray(read_from_csv("gmi", directory=str(tmp_path)))
    assert back.shape == (1 + 4 * fsl.N_IDX, 3)
    np.testing.assert_array_equal(back[0], ebn0)
    n = 5 * fsl.N_SC * 4
    for k in range(fsl.N_IDX):
        bad = math.floor(n / (4 + 4 * k + 4.0))
        np.testing.assert_allclose(back[1 + 4 * k], [bad / n] * 3, rtol=1e-15)
        for j in range(3):
            st = stats[1][j]
            s = back[3 + 4 * k, j]
            assert s == pytest.approx(st.best_scale()[k], rel=1e-12)
            c_good = round(snr[j]) + 0.5
            want = 1 - (bad * f2(-0.5 * s) + (n - bad) * f2(c_good * s)) / n
            assert back[2 + 4 * k, j] == pytest.approx(want, rel=1e-12)
            assert back[4 + 4 * k, j] == pytest.approx(4 * want, rel=1e-12)
