"""Spectrum mode on a machine without a GPU: the width helper, the host-side argument checks of
mimo_engine_spectrum_points (no HIP call before them), SpectrumStats arithmetic on hand-made rows,
and sweep.spectrum_vs_ibo with the psd_vs_ibo CSV writers against a fake link."""
import ctypes
import warnings

import numpy as np
import pytest

import _engine
import fake_spectrum_link as fsl
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


def _spectrum(lib, h, iters, spec, n_trials=8):
    pt = _engine.Engine.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9)
    it = np.asarray(iters, np.int32)
    one = lambda v: np.asarray([v], np.uint64)  # noqa: E731
    seeds, first, n = one(1), one(0), one(n_trials)
    err = np.zeros(8, np.uint64)
    bits = np.zeros(8, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_spectrum_points(h, 1, ctypes.byref(pt), seeds.ctypes.data_as(u64), first.ctypes.data_as(u64),
                                         n.ctypes.data_as(u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         len(it), 0, err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None,
                                         spec.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if spec is not None
                                         else None, None)
    return rc, lib.mimo_last_error().decode()


def test_spectrum_width():
    lib = _engine.lib()
    assert _engine.SPEC_FIXED == 3
    assert lib.mimo_spectrum_width(256) == 259
    for f in (128, 512, 1024, 2048, 4096, 8192):
        assert lib.mimo_spectrum_width(f) == f + 3
    for bad in (100, 16384):
        assert lib.mimo_spectrum_width(bad) == -1  # MIMO_EINVAL
        assert "n_fft" in lib.mimo_last_error().decode()


def test_spectrum_rejects_float32_engine_before_any_hip_call():
    lib, h, keep = _engine_handle(precision=1)
    spec = np.full(515, 7.0)
    rc, msg = _spectrum(lib, h, [0], spec)
    assert rc == -1 and "float64" in msg and "spectrum" in msg, (rc, msg)
    assert np.all(spec == 7.0)  # nothing added
    lib.mimo_engine_destroy(h)


def test_spectrum_rejects_null_spec_out_before_any_hip_call():
    lib, h, keep = _engine_handle()
    rc, msg = _spectrum(lib, h, [0], None)
    assert rc == -1 and "spec_out" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)


def test_spectrum_rejects_bad_iters_before_any_hip_call():
    lib, h, keep = _engine_handle()
    spec = np.full(515, 7.0)
    rc, msg = _spectrum(lib, h, [2, 1], spec)
    assert rc == -1 and "sorted and unique" in msg, (rc, msg)
    assert np.all(spec == 7.0)
    lib.mimo_engine_destroy(h)


def test_inband_bins_restate_the_oracle():
    for f, s in ((16, 8), (256, 100), (512, 256), (8192, 4096)):
        np.testing.assert_array_equal(_engine.inband_bins(f, s), rm.inband_bins(f, s))


# F 16, S 8: in-band bins 12 .. 15 and 1 .. 4; DC (bin 0) and bins 5 .. 11 are out of band
HAND_PSD = np.array([0.5, 4.0, 4.0, 2.0, 2.0, 0.25, 0.125, 0.0, 0.0, 0.0, 0.0, 0.125, 1.0, 1.0, 1.0, 1.0])


def hand_row(ex=20.0, c=complex(12.0, -9.0)):
    return np.concatenate([HAND_PSD, [ex, c.real, c.imag]])


def test_spectrum_stats_exact_values():
    st = _engine.SpectrumStats(hand_row(), 8, n_trials=2)
    assert (st.n_fft, st.n_sub_carr, st.n_trials) == (16, 8, 2)
    np.testing.assert_array_equal(st.psd, HAND_PSD)
    assert st.total == 17.0
    assert st.inband == 16.0              # 4 + 4 + 2 + 2 + 4 x 1
    assert st.oob == 1.0                  # the DC bin's 0.5 counts as out of band
    assert st.oob_ratio_db == pytest.approx(10 * np.log10(1.0 / 17.0), abs=1e-12)
    assert (st.ex, st.c) == (20.0, complex(12.0, -9.0))
    assert st.gain == complex(0.6, -0.45)
    assert st.efficiency == 17.0 / 20.0
    # |C|^2 / Ex = 225 / 20 = 11.25 of the 16 in band are correlated with the input
    assert st.radiated_sdr_db == pytest.approx(10 * np.log10(11.25 / 4.75), abs=1e-12)
    # mean in-band psd = 2
    rel = st.psd_rel_db
    assert rel[1] == pytest.approx(10 * np.log10(2.0), abs=1e-12) and rel[12] == pytest.approx(-10 * np.log10(2.0))
    assert rel[7] == -np.inf
    # centred order: bins 8 .. 15 (frequencies -8 .. -1), then 0 .. 7
    np.testing.assert_array_equal(st.freq_index, np.arange(-8, 8))
    np.testing.assert_array_equal(st.psd_centered, np.concatenate([HAND_PSD[8:], HAND_PSD[:8]]))
    assert st.psd_centered[8] == 0.5 and st.freq_index[8] == 0  # DC in the middle


def test_spectrum_stats_edges_without_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        row = np.zeros(19)
        row[rm.inband_bins(16, 8)] = 2.0
        row[16:] = [16.0, 16.0, 0.0]  # a linear array: Y = X
        st = _engine.SpectrumStats(row, 8)
        assert st.oob == 0.0 and st.oob_ratio_db == -np.inf
        assert st.radiated_sdr_db == np.inf and st.gain == 1.0 and st.efficiency == 1.0
        assert np.all(st.psd_rel_db[rm.inband_bins(16, 8)] == 0.0)
        # rounding may leave inband - |C|^2 / Ex a hair below zero: still inf
        row[17] = 16.0 + 1e-12
        assert _engine.SpectrumStats(row, 8).radiated_sdr_db == np.inf
    with pytest.raises(ValueError, match="n_fft"):
        _engine.SpectrumStats(np.ones(19), 16)


def test_spectrum_stats_pooling_is_the_row_sum():
    rng = np.random.default_rng(5)
    rows = rng.uniform(1.0, 2.0, (3, 19))
    parts = [_engine.SpectrumStats(rows[i], 8, n_trials=i + 1) for i in range(3)]
    pooled = parts[0] + parts[1] + parts[2]
    direct = _engine.SpectrumStats((rows[0] + rows[1]) + rows[2], 8)
    np.testing.assert_array_equal(pooled.row, direct.row)
    assert pooled.n_trials == 6
    assert pooled.oob_ratio_db == direct.oob_ratio_db and pooled.gain == direct.gain
    assert (parts[0] + _engine.SpectrumStats(rows[1], 8)).n_trials is None
    with pytest.raises(ValueError, match="different systems"):
        parts[0] + _engine.SpectrumStats(np.ones(35), 8)
    with pytest.raises(ValueError, match="different systems"):
        parts[0] + _engine.SpectrumStats(rows[1], 4)


def test_spectrum_vs_ibo_and_csv_writers(tmp_path):
    import sweep
    from utilities import read_from_csv, save_to_csv
    link = fsl.FakeSpectrumLink()
    ibos = np.array([0.0, 3.0, 6.0])
    stats = sweep.spectrum_vs_ibo(link, ibos, 5, seed=11)
    assert len(link.calls) == 1  # every point in one call
    call = link.calls[0]
    assert call["ibos"] == [0.0, 3.0, 6.0] and call["n_trials"] == 5 and call["reroll_chan"] is True
    assert call["seeds"] == [sweep.point_seed(11, i) for i in range(3)]
    for ibo, st in zip(ibos, stats):
        np.testing.assert_array_equal(st.row, fsl.fake_row(ibo, 5))
    # summary: one row per IBO
    rows = sweep.oob_vs_ibo_rows(ibos, stats)
    save_to_csv(rows, "oob", directory=str(tmp_path))
    back = np.asarray(read_from_csv("oob", directory=str(tmp_path)))
    assert back.shape == (3, 5)
    for i, ibo in enumerate(ibos):
        q = 10.0 ** (-(20.0 + ibo) / 10.0)  # out-of-band bins over in-band bins; 8 of each
        g = 1.0 - 0.1 / (1.0 + ibo)
        want = [ibo, 10 * np.log10(q / (1 + q)), 10 * np.log10(g * g * 1.25 * 0.5 / (1 - g * g * 1.25 * 0.5)),
                g * 0.5 * np.sqrt(1.25), (1 + q) / 2]
        np.testing.assert_allclose(back[i], want, rtol=1e-12)
    # PSD: one row per centred bin, one column per IBO after the bin index
    save_to_csv(sweep.psd_vs_ibo_rows(stats), "psd", directory=str(tmp_path))
    back = np.asarray(read_from_csv("psd", directory=str(tmp_path)))
    assert back.shape == (16, 4)
    np.testing.assert_array_equal(back[:, 0], np.arange(-8, 8))
    inband = np.isin(np.arange(-8, 8), [-4, -3, -2, -1, 1, 2, 3, 4])
    for i, ibo in enumerate(ibos):
        np.testing.assert_allclose(back[inband, 1 + i], 0.0, atol=1e-12)
        np.testing.assert_allclose(back[~inband, 1 + i], -(20.0 + ibo), rtol=1e-12)
