"""Measure mode on a machine without a GPU: the width helper, the host-side argument checks of
mimo_engine_measure_points (no HIP call before them), SignalStats arithmetic on hand-made rows,
and the report a library without the new entry points gets."""
import ctypes
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import _engine


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


def _measure(lib, h, iters, meas, n_trials=8):
    pt = _engine.Engine.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9)
    it = np.asarray(iters, np.int32)
    one = lambda v: np.asarray([v], np.uint64)  # noqa: E731
    seeds, first, n = one(1), one(0), one(n_trials)
    err = np.zeros(8, np.uint64)
    bits = np.zeros(8, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_measure_points(h, 1, ctypes.byref(pt), seeds.ctypes.data_as(u64), first.ctypes.data_as(u64),
                                        n.ctypes.data_as(u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        len(it), 0, err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None,
                                        meas.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if meas is not None
                                        else None, None)
    return rc, lib.mimo_last_error().decode()


def test_measure_width():
    lib = _engine.lib()
    assert _engine.MEAS_FIXED == 5
    for n_iters, clean in ((1, 0), (1, 1), (3, 0), (9, 1), (32, 1)):
        assert lib.mimo_measure_width(n_iters, clean) == 5 + n_iters + clean
    assert lib.mimo_measure_width(0, 0) == -1  # MIMO_EINVAL
    assert "n_iters" in lib.mimo_last_error().decode()


def test_measure_rejects_float32_engine_before_any_hip_call():
    lib, h, keep = _engine_handle(precision=1)
    rc, msg = _measure(lib, h, [0, 1], np.zeros(7))
    assert rc == -1 and "float64" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)


def test_measure_rejects_null_meas_out_before_any_hip_call():
    lib, h, keep = _engine_handle()
    rc, msg = _measure(lib, h, [0, 1], None)
    assert rc == -1 and "meas_out" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("iters,msg", [([2, 1], "sorted and unique"), ([32], "[0, 31]"), ([], "at least one iteration")])
def test_measure_rejects_bad_iters_before_any_hip_call(iters, msg):
    lib, h, keep = _engine_handle()
    meas = np.full(16, 7.0)
    rc, text = _measure(lib, h, iters, meas)
    assert rc == -1 and msg in text, (rc, text)
    assert np.all(meas == 7.0)  # nothing added
    lib.mimo_engine_destroy(h)


def test_signal_stats_exact_values():
    # z0 = beta s + d with beta = 0.5 - 0.5j, Es = 100, |d|^2 total 0.5 uncorrelated with s:
    # C = beta Es, Ez0 = |beta|^2 Es + 0.5 = 50.5
    st = _engine.SignalStats([100.0, 50.5, 50.0, -50.0, 10.0, 1.0, 0.1, 100.0], err=[5, 0, 50], bits=[1000, 1000, 1000])
    assert st.gain == complex(0.5, -0.5)
    assert st.sdr_db == pytest.approx(10 * np.log10(5000.0 / 50.0), abs=1e-12)   # 20 dB
    assert st.slicer_sdr_db == pytest.approx(10.0, abs=1e-12)
    np.testing.assert_allclose(st.sndr_db, [20.0, 30.0, 0.0], atol=1e-12)
    np.testing.assert_array_equal(st.ber, [0.005, 0.0, 0.05])
    assert (st.es, st.ez0, st.c, st.ed0) == (100.0, 50.5, complex(50.0, -50.0), 10.0)
    st2 = _engine.SignalStats.from_totals(100.0, 50.5, complex(50.0, -50.0), 10.0, [1.0, 0.1, 100.0])
    np.testing.assert_array_equal(st2.row, st.row)


def test_signal_stats_zero_distortion_is_inf_without_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st = _engine.SignalStats([100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 4.0])
        assert st.sdr_db == np.inf and st.slicer_sdr_db == np.inf
        sndr = st.sndr_db
        assert sndr[0] == np.inf and sndr[1] == pytest.approx(10 * np.log10(25.0))
        assert not np.any(np.isnan(sndr)) and not np.any(np.isnan(st.ber))
        assert np.all(st.ber == 0.0)  # no bits recorded: 0, not NaN
        # rounding may leave Es Ez0 - |C|^2 a hair below zero: still inf
        assert _engine.SignalStats([100.0, 100.0 - 1e-13, 100.0, 0.0, 0.0, 1.0]).sdr_db == np.inf


def test_signal_stats_pooling_is_the_row_sum():
    rng = np.random.default_rng(5)
    rows = rng.uniform(1.0, 2.0, (3, 8))
    rows[:, 1] += 4.0  # Es Ez0 > |C|^2
    errs = rng.integers(0, 100, (3, 3))
    bits = np.full((3, 3), 600)
    parts = [_engine.SignalStats(rows[i], errs[i], bits[i]) for i in range(3)]
    pooled = parts[0] + parts[1] + parts[2]
    direct = _engine.SignalStats((rows[0] + rows[1]) + rows[2], errs.sum(0), bits.sum(0))
    np.testing.assert_array_equal(pooled.row, direct.row)
    np.testing.assert_array_equal(pooled.err, direct.err)
    np.testing.assert_array_equal(pooled.bits, direct.bits)
    assert pooled.sdr_db == direct.sdr_db and pooled.gain == direct.gain
    np.testing.assert_array_equal(pooled.sndr_db, direct.sndr_db)
    with pytest.raises(ValueError, match="counter layouts"):
        parts[0] + _engine.SignalStats(np.ones(7))


def test_abi8_library_without_measure_is_reported_by_name(tmp_path, monkeypatch):
    """The measure entry points were added within ABI 8: a library that answers 8 and exports
    nothing else is reported as lacking a named entry point ('rebuild it'), not bound blindly."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [n for n in _engine.SYMBOLS if n not in ("mimo_measure_width", "mimo_engine_measure_points")]
    src = tmp_path / "stale.c"
    src.write_text("int mimo_abi_version(void) { return 8; }\n" +
                   "".join(f"void {n}(void) {{}}\n" for n in names if n != "mimo_abi_version"))
    so = tmp_path / "libstale8.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(so))
    with pytest.raises(_engine.EngineError, match=r"\(ABI 8\) lacks mimo_measure_width: rebuild it"):
        _engine.lib()
    # ... and the bare stub of the issue: ABI 8 and nothing else
    src.write_text("int mimo_abi_version(void) { return 8; }\n")
    so2 = tmp_path / "libbare8.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so2), str(src)], check=True)
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(so2))
    with pytest.raises(_engine.EngineError, match=r"\(ABI 8\) lacks \w+: rebuild it"):
        _engine.lib()
