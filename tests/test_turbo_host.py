"""Host side of the turbo mode (mimo_engine_turbo_points, mimo_engine_cnc_step), no GPU: the width
function, every argument the entry points refuse before any HIP call with the message that names it,
TurboStats' arithmetic, and sweep.turbo_ber_vs_ebn0 with its CSV writer against a fake link."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import _engine
import fake_turbo_link as ftl
from test_coded_host import BROKEN, good_code
from utilities import qc_ldpc_code

DP = ctypes.POINTER(ctypes.c_double)


def _engine_handle(precision=0, receiver=1):
    lib = _engine.lib()
    tx = np.zeros((4, 3))
    fr = np.full(512, 3.5e9)
    c = _engine.MimoConfig(n_ant=4, n_sub_carr=256, n_fft=512, constel_size=16, cp_len=16, channel_kind=1,
                           receiver_kind=receiver, device=-1, rx_loc_var=10.0, reroll_chan=1, precision=precision,
                           tx_pos=tx.ctypes.data_as(DP), carrier_freqs=fr.ctypes.data_as(DP))
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h
    return lib, h, (tx, fr)


def _point():
    return _engine.Engine.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9)


def _turbo(lib, h, code, out, rho_max=16.0, n_passes=3, iters=(0,), n_trials=8):
    """One turbo call of the S 256, 16-QAM engine (1,024 bits per trial) -> (rc, message)."""
    pt = _point()
    it = np.asarray(iters, np.int32)
    one = lambda v: np.asarray([v], np.uint64)  # noqa: E731
    seeds, first, n = one(1), one(0), one(n_trials)
    err = np.zeros(40, np.uint64)
    bits = np.zeros(40, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_turbo_points(h, 1, ctypes.byref(pt), seeds.ctypes.data_as(u64), first.ctypes.data_as(u64),
                                      n.ctypes.data_as(u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      len(it), 0, err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None,
                                      ctypes.byref(code) if code is not None else None, ctypes.c_double(rho_max),
                                      n_passes, out.ctypes.data_as(DP) if out is not None else None, None, None, None)
    return rc, lib.mimo_last_error().decode()


def _step(lib, h, pt, z, labels, n, v):
    rc = lib.mimo_engine_cnc_step(h, ctypes.byref(pt) if pt is not None else None,
                                  z.ctypes.data_as(DP) if z is not None else None,
                                  labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if labels is not None else None,
                                  n, v.ctypes.data_as(DP) if v is not None else None)
    return rc, lib.mimo_last_error().decode()


# ---------------------------------------------------------------- width
def test_turbo_width():
    lib = _engine.lib()
    assert _engine.TURBO_MAX_PASSES == 16
    assert [lib.mimo_turbo_width(n) for n in (1, 3, 16)] == [4, 12, 64]
    assert _engine.turbo_width(4) == 16
    for bad in (0, -1, 17):
        assert lib.mimo_turbo_width(bad) == -1 and "n_passes" in lib.mimo_last_error().decode()
        with pytest.raises(_engine.EngineError, match=r"n_passes must be in \[1, 16\]"):
            _engine.turbo_width(bad)


# ---------------------------------------------------------------- what the call refuses, before any HIP call (no GPU here)
@pytest.mark.parametrize("name,code,word", BROKEN, ids=[b[0] for b in BROKEN])
def test_every_code_rule_is_refused_by_name(name, code, word):
    lib, h, keep = _engine_handle()
    out = np.full(12, 7.0)
    rc, msg = _turbo(lib, h, code, out)
    assert rc == -1 and word in msg, (rc, msg)
    assert np.all(out == 7.0)  # nothing added
    lib.mimo_engine_destroy(h)


def test_turbo_rejects_float32_mcnc_null_code_and_null_out():
    out = np.full(12, 7.0)
    lib, h, keep = _engine_handle(precision=1)
    rc, msg = _turbo(lib, h, good_code(), out)
    assert rc == -1 and "float64" in msg and "turbo" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)
    lib, h, keep = _engine_handle(receiver=2)
    rc, msg = _turbo(lib, h, good_code(), out)
    assert rc == -1 and "receiver_kind" in msg and "MIMO_RX_CNC" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)
    lib, h, keep = _engine_handle()
    rc, msg = _turbo(lib, h, None, out)
    assert rc == -1 and "null code" in msg, (rc, msg)
    rc, msg = _turbo(lib, h, good_code(), None)
    assert rc == -1 and "turbo_out" in msg, (rc, msg)
    assert lib.mimo_engine_turbo_points(None, 0, None, None, None, None, None, 0, 0, None, None, None, None,
                                        ctypes.c_double(1.0), 1, None, None, None, None) == -1
    assert "null engine" in lib.mimo_last_error().decode()
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("n_passes", [0, -3, 17, 1 << 20])
def test_turbo_rejects_n_passes_out_of_range(n_passes):
    lib, h, keep = _engine_handle()
    out = np.full(64, 7.0)
    rc, msg = _turbo(lib, h, good_code(), out, n_passes=n_passes)
    assert rc == -1 and "n_passes must be in [1, 16]" in msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("rho_max", [0.0, -1.0, float("nan"), float("inf"), 1e-320])
def test_turbo_rejects_bad_rho_max(rho_max):
    lib, h, keep = _engine_handle()
    out = np.full(12, 7.0)
    rc, msg = _turbo(lib, h, good_code(), out, rho_max)
    assert rc == -1 and "rho_max" in msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


def test_turbo_rejects_a_code_longer_than_a_trial_and_bad_iters():
    lib, h, keep = _engine_handle()   # 1,024 bits per trial
    out = np.full(12, 7.0)
    rc, msg = _turbo(lib, h, qc_ldpc_code(256, 2, 5), out)   # N 1,280
    assert rc == -1 and "1280" in msg and "1024" in msg, (rc, msg)
    for iters in ([2, 1], [], list(range(33))):
        rc, msg = _turbo(lib, h, good_code(), out, iters=iters)
        assert rc == -1 and msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


def test_python_wrapper_passes_the_refusals_on():
    eng = _engine.Engine(4, 256, 512, 16, 16, "rayleigh", "mcnc", np.zeros((4, 3)), [1.0, 2.0, 3.0], 10.0,
                         np.full(512, 3.5e9), precision="f64")
    with pytest.raises(_engine.EngineError, match="receiver_kind"):
        eng.turbo(1, 0, 4, (0,), good_code(), 16.0, 2, point=_point())
    with pytest.raises(_engine.EngineError, match="receiver_kind"):
        eng.cnc_step(np.zeros((1, 256), complex), np.zeros((1, 256), int), point=_point())
    eng.close()
    eng = _engine.Engine(4, 256, 512, 16, 16, "rayleigh", "cnc", np.zeros((4, 3)), [1.0, 2.0, 3.0], 10.0,
                         np.full(512, 3.5e9), precision="f64")
    for bad in (17, 0, -2):  # the library's refusal, whatever the wrapper allocated
        with pytest.raises(_engine.EngineError, match=r"n_passes must be in \[1, 16\]"):
            eng.turbo(1, 0, 4, (0,), good_code(), 16.0, bad, point=_point(), chan=True, z=True)
        with pytest.raises(_engine.EngineError, match=r"n_passes must be in \[1, 16\]"):
            eng.turbo(1, 0, 4, (0,), good_code(), 16.0, bad, point=_point())
    with pytest.raises(_engine.EngineError, match="set_point"):
        eng.cnc_step(np.zeros((1, 256), complex), np.zeros((1, 256), int))
    with pytest.raises(ValueError, match="n_sub_carr"):
        eng.cnc_step(np.zeros((2, 256), complex), np.zeros((1, 256), int), point=_point())
    eng.close()


# ---------------------------------------------------------------- the seam's refusals
def test_cnc_step_refusals():
    z, lab, v = np.zeros(2 * 256 * 2), np.zeros(2 * 256, np.int32), np.full(2 * 256 * 2, 7.0)
    lib, h, keep = _engine_handle(precision=1)
    rc, msg = _step(lib, h, _point(), z, lab, 2, v)
    assert rc == -1 and "float64" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)
    lib, h, keep = _engine_handle(receiver=2)
    rc, msg = _step(lib, h, _point(), z, lab, 2, v)
    assert rc == -1 and "MIMO_RX_CNC" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)
    lib, h, keep = _engine_handle()
    rc, msg = _step(lib, None, _point(), z, lab, 2, v)
    assert rc == -1 and "null engine" in msg
    rc, msg = _step(lib, h, None, z, lab, 2, v)
    assert rc == -1 and "null point" in msg
    bad_pt = _point()
    bad_pt.cnc_alpha = 0.0
    rc, msg = _step(lib, h, bad_pt, z, lab, 2, v)
    assert rc == -1 and "cnc_alpha" in msg
    for n in (-1, (1 << 20) + 1):
        rc, msg = _step(lib, h, _point(), z, lab, n, v)
        assert rc == -1 and "n must be in" in msg
    for args in ((None, lab, v), (z, None, v), (z, lab, None)):
        rc, msg = _step(lib, h, _point(), args[0], args[1], 2, args[2])
        assert rc == -1 and "null z_iq, labels or v_out" in msg
    for at, bad in ((0, -1), (300, 16), (511, 1 << 30)):
        lab2 = lab.copy()
        lab2[at] = bad
        rc, msg = _step(lib, h, _point(), z, lab2, 2, v)
        assert rc == -1 and f"labels[{at}]" in msg and "constel_size" in msg, (rc, msg)
    assert _step(lib, h, _point(), None, None, 0, None)[0] == 0   # n = 0: MIMO_OK, nothing touched
    assert np.all(v == 7.0)
    lib.mimo_engine_destroy(h)


def test_abi8_library_without_turbo_is_reported_by_name(tmp_path, monkeypatch):
    """The turbo entry points were added within ABI 8: a library that answers 8 and exports everything
    but them is reported as lacking a named entry point ('rebuild it')."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    mine = ("mimo_turbo_width", "mimo_engine_turbo_points", "mimo_engine_cnc_step")
    assert all(n in _engine.SYMBOLS for n in mine)
    names = [n for n in _engine.SYMBOLS if n not in mine]
    src = tmp_path / "stale.c"
    src.write_text("int mimo_abi_version(void) { return 8; }\n" +
                   "".join(f"void {n}(void) {{}}\n" for n in names if n != "mimo_abi_version"))
    so = tmp_path / "libstale8.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(so))
    with pytest.raises(_engine.EngineError, match=r"\(ABI 8\) lacks mimo_turbo_width: rebuild it"):
        _engine.lib()


# ---------------------------------------------------------------- TurboStats
def test_turbo_stats_arithmetic():
    cells = np.array([[1191.0, 102.0, 3.0, 3.0], [183.0, 0.0, 0.0, 0.0], [144.0, 5.0, 2.0, 1.0]])
    st = _engine.TurboStats(cells, 24, 512)
    assert (st.n_passes, st.n_frames, st.n_code_bits, st.n_bits) == (3, 24, 512, 12288)
    np.testing.assert_array_equal(st.raw_ber(), cells[:, 0] / 12288)
    np.testing.assert_array_equal(st.ber(), cells[:, 1] / 12288)
    np.testing.assert_array_equal(st.fer(), cells[:, 2] / 24)
    np.testing.assert_array_equal(st.syndrome_rate(), cells[:, 3] / 24)
    np.testing.assert_array_equal(st.undetected(), (cells[:, 2] - cells[:, 3]) / 24)
    both = st + _engine.TurboStats(cells[::-1], 6, 512)
    assert both.n_frames == 30
    np.testing.assert_array_equal(both.cells, cells + cells[::-1])
    with pytest.raises(ValueError):
        st + _engine.TurboStats(cells, 24, 513)
    with pytest.raises(ValueError):
        st + _engine.TurboStats(cells[:2], 24, 512)
    with pytest.raises(TypeError):
        st + _engine.CodedStats(cells, 24, 512)
    with pytest.raises(ValueError, match="n_passes"):
        _engine.TurboStats(np.zeros((17, 4)), 1, 512)
    empty = _engine.TurboStats(np.zeros((2, 4)), 0, 96)
    assert np.all(empty.ber() == 0) and np.all(empty.fer() == 0)
    flat = _engine.TurboStats(cells.reshape(-1), 24, 512)  # a flat row of n_passes * 4 cells
    np.testing.assert_array_equal(flat.cells, cells)
    assert "n_passes=3" in repr(st) and "fer=" in repr(st)


# ---------------------------------------------------------------- the sweep grid on a fake link
def test_turbo_ber_vs_ebn0_and_csv_writer(tmp_path):
    import sweep
    from utilities import ebn0_to_snr, read_from_csv, save_to_csv
    link = ftl.FakeTurboLink()
    code = good_code()
    ibos, ebn0 = np.array([0.0, 4.0]), np.array([6.0, 10.0, 14.0])
    stats = sweep.turbo_ber_vs_ebn0(link, ibos, ebn0, 3, 5, code, seed=11)
    snr = [float(v) for v in ebn0_to_snr(ebn0, ftl.N_SC, ftl.N_SC, ftl.M)]
    assert len(link.calls) == 3  # the IBOs of one Eb/N0 in one call
    for j, call in enumerate(link.calls):
        assert call["ibos"] == [0.0, 4.0] and call["snrs"] == [snr[j]] * 2 and call["n_trials"] == 5
        assert call["n_passes"] == 3 and call["reroll_chan"] is True
        assert call["rho_max"] is None and call["code"] is code
        assert call["seeds"] == [sweep.point_seed(11, i * 3 + j) for i in range(2)]  # the coded grid's seeds
    assert len(stats) == 2 and all(len(r) == 3 for r in stats)
    for i, ibo in enumerate(ibos):
        for j in range(3):
            np.testing.assert_array_equal(stats[i][j].cells, ftl.fake_cells(ibo, snr[j], 5, 3))
    sweep.turbo_ber_vs_ebn0(link, ibos[:1], ebn0[:1], 1, 2, code, seed=11, reroll_chan=False, rho_max=4.0)
    assert link.calls[3]["rho_max"] == 4.0 and link.calls[3]["reroll_chan"] is False and link.calls[3]["n_passes"] == 1
    rows = sweep.turbo_ber_vs_ebn0_rows(ebn0, stats[1])
    save_to_csv(rows, "turbo", directory=str(tmp_path))
    back = np.asarray(read_from_csv("turbo", directory=str(tmp_path)))
    assert back.shape == (1 + 4 * 3, 3)
    np.testing.assert_array_equal(back[0], ebn0)
    frames = 5 * ftl.N_CW
    bits = frames * ftl.N_CODE_BITS
    for q in range(3):
        for j in range(3):
            c = ftl.fake_cells(4.0, snr[j], 5, 3)[q]
            assert back[1 + 4 * q, j] == c[0] / bits and back[2 + 4 * q, j] == c[1] / bits
            assert back[3 + 4 * q, j] == c[2] / frames and back[4 + 4 * q, j] == c[3] / frames


def test_sweep_parser_knows_the_grid():
    import sweep
    args = sweep.build_parser().parse_args(["--grid", "turbo_ber_vs_ebn0", "--turbo-passes", "4"])
    assert args.grid == "turbo_ber_vs_ebn0" and args.turbo_passes == 4 and args.ldpc == "128,4,8,10"
