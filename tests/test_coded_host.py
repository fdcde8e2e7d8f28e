"""Host side of the coded mode (mimo_engine_coded_points, mimo_ldpc_decode), no GPU: every argument
the entry points refuse before any HIP call, the width and codeword functions, the stand-in code
constructor utilities.qc_ldpc_code, CodedStats' arithmetic, the numpy reference decoder's own
properties (tests/ldpc_ref.py: a clean input stays clean, and decoding commutes with the sign flips
of a codeword), and sweep.coded_ber_vs_ebn0 with its CSV writer against a fake link."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import _engine
import fake_coded_link as fcl
import ldpc_ref
from utilities import qc_ldpc_code


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


def _coded(lib, h, code, out, rho_max=16.0, iters=(0,), n_trials=8):
    """One coded call of the S 256, 16-QAM engine (1,024 bits per trial) -> (rc, message)."""
    pt = _engine.Engine.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9)
    it = np.asarray(iters, np.int32)
    one = lambda v: np.asarray([v], np.uint64)  # noqa: E731
    seeds, first, n = one(1), one(0), one(n_trials)
    err = np.zeros(40, np.uint64)
    bits = np.zeros(40, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_coded_points(h, 1, ctypes.byref(pt), seeds.ctypes.data_as(u64), first.ctypes.data_as(u64),
                                      n.ctypes.data_as(u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      len(it), 0, err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None,
                                      ctypes.byref(code) if code is not None else None, ctypes.c_double(rho_max),
                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if out is not None else None,
                                      None, None)
    return rc, lib.mimo_last_error().decode()


def good_code():
    return qc_ldpc_code(16, 3, 6)


def raw_code(z, shifts, n_dec_iters=10, n_rows=None, n_cols=None):
    """An LdpcCode whose fields may break the rules (the constructor only marshals)."""
    c = _engine.LdpcCode(z, shifts, n_dec_iters)
    if n_rows is not None:
        c.n_rows = n_rows
    if n_cols is not None:
        c.n_cols = n_cols
    return c


def broken_codes():
    """(name, code, word the message must hold) of every rule of mimo_ldpc_code, one broken at a time."""
    s = np.array(good_code().table)
    punched_row = s.copy()
    punched_row[1, 1:] = -1            # base row 1 keeps weight 1
    punched_col = s.copy()
    punched_col[:, 2] = -1             # base column 2 keeps weight 0
    wide = np.zeros((1, 33), np.int16)  # one base row of weight 33
    out = [("z0", raw_code(0, s), "code.z"), ("z513", raw_code(513, s), "code.z"),
           ("rows0", raw_code(16, s, n_rows=0), "code.n_rows"), ("rows65", raw_code(16, s, n_rows=65), "code.n_rows"),
           ("cols1", raw_code(16, s, n_cols=1), "code.n_cols"), ("cols129", raw_code(16, s, n_cols=129), "code.n_cols"),
           ("it0", raw_code(16, s, 0), "code.n_dec_iters"), ("it65", raw_code(16, s, 65), "code.n_dec_iters"),
           ("shift_z", raw_code(16, np.where(s == s[0, 0], 16, s)), "shifts"),
           ("shift_m2", raw_code(16, np.where(s == s[0, 0], -2, s)), "shifts"),
           ("row_w1", raw_code(16, punched_row), "row 1"), ("row_w33", raw_code(2, wide), "row 0"),
           ("col_w0", raw_code(16, punched_col), "column 2")]
    null_shifts = good_code()
    null_shifts.shifts = None
    out.append(("null_shifts", null_shifts, "shifts"))
    return out


BROKEN = broken_codes()


# ---------------------------------------------------------------- width, codewords
def test_coded_width_and_codewords():
    lib = _engine.lib()
    assert _engine.CODED_FIXED == 4 == ldpc_ref.CODED_FIXED
    assert lib.mimo_coded_width(1, 0) == 4 and lib.mimo_coded_width(3, 1) == 16 and lib.mimo_coded_width(32, 1) == 132
    assert _engine.coded_width(2, True) == 12
    for bad in (0, -1, 33):
        assert lib.mimo_coded_width(bad, 0) == -1 and "n_iters" in lib.mimo_last_error().decode()
    code = good_code()  # N 96
    assert code.n_bits == 96
    assert _engine.coded_codewords(64, 4, code) == 1       # 128 bits: 32 left over
    assert _engine.coded_codewords(100, 64, code) == 6     # 600 bits: 24 left over
    assert _engine.coded_codewords(16, 64, code) == 1      # exactly one
    assert _engine.coded_codewords(100, 64, qc_ldpc_code(61, 3, 6)) == 1 == ldpc_ref.n_codewords(
        100, 64, ldpc_ref.Code(61, qc_ldpc_code(61, 3, 6).table))
    with pytest.raises(_engine.EngineError, match="exceed"):
        _engine.coded_codewords(12, 64, code)              # 72 bits < N
    with pytest.raises(_engine.EngineError, match="Constellation"):
        _engine.coded_codewords(64, 8, code)
    with pytest.raises(_engine.EngineError, match="null code"):
        _engine.coded_codewords(64, 4, None)


@pytest.mark.parametrize("name,code,word", BROKEN, ids=[b[0] for b in BROKEN])
def test_every_code_rule_is_refused_by_name(name, code, word):
    """... by mimo_coded_codewords, mimo_engine_coded_points and mimo_ldpc_decode alike, before any HIP
    call (no GPU here), with a message that names the field."""
    lib, h, keep = _engine_handle()
    assert lib.mimo_coded_codewords(256, 16, ctypes.byref(code)) == -1
    assert word in lib.mimo_last_error().decode(), lib.mimo_last_error().decode()
    out = np.full(4, 7.0)
    rc, msg = _coded(lib, h, code, out)
    assert rc == -1 and word in msg, (rc, msg)
    assert np.all(out == 7.0)  # nothing added
    chan = np.ones(4096, np.int8)
    app = np.zeros(4096, np.int16)
    rc = lib.mimo_ldpc_decode(ctypes.byref(code), chan.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), 1,
                              app.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)))
    assert rc == -1 and word in lib.mimo_last_error().decode()
    lib.mimo_engine_destroy(h)


def test_coded_rejects_float32_engine_null_code_and_null_out():
    lib, h, keep = _engine_handle(precision=1)
    out = np.full(4, 7.0)
    rc, msg = _coded(lib, h, good_code(), out)
    assert rc == -1 and "float64" in msg and "coded" in msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)
    lib, h, keep = _engine_handle()
    rc, msg = _coded(lib, h, None, out)
    assert rc == -1 and "null code" in msg, (rc, msg)
    rc, msg = _coded(lib, h, good_code(), None)
    assert rc == -1 and "coded_out" in msg, (rc, msg)
    lib.mimo_engine_destroy(h)


def test_coded_rejects_a_code_longer_than_a_trial():
    lib, h, keep = _engine_handle()   # 1,024 bits per trial
    out = np.full(4, 7.0)
    rc, msg = _coded(lib, h, qc_ldpc_code(256, 2, 5), out)   # N 1,280
    assert rc == -1 and "1280" in msg and "1024" in msg, (rc, msg)
    rc, msg = _coded(lib, h, qc_ldpc_code(256, 2, 4), out, rho_max=float("nan"))  # N 1,024 fits: the next rule
    assert rc == -1 and "rho_max" in msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("rho_max", [0.0, -1.0, float("nan"), float("inf"), float("-inf"), 1e-320])
def test_coded_rejects_bad_rho_max_before_any_hip_call(rho_max):
    lib, h, keep = _engine_handle()
    out = np.full(4, 7.0)
    rc, msg = _coded(lib, h, good_code(), out, rho_max)
    assert rc == -1 and "rho_max" in msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("iters", [[2, 1], [], list(range(33))])
def test_coded_rejects_bad_iters_before_any_hip_call(iters):
    lib, h, keep = _engine_handle()
    out = np.full(4 * 34, 7.0)
    rc, msg = _coded(lib, h, good_code(), out, iters=iters)
    assert rc == -1 and msg, (rc, msg)
    assert np.all(out == 7.0)
    lib.mimo_engine_destroy(h)


def test_decoder_state_beyond_the_lds_is_refused_with_the_byte_figure():
    """2 B per code bit (to a multiple of 8) + 8 B per check + 96 B against 163,840 B: z 512, 12 x 24
    (73,824 B) is accepted by the host checks, z 512 with 40 rows of 2 columns (2,048 + 163,840 + 96)
    is not."""
    lib = _engine.lib()
    fits = qc_ldpc_code(512, 12, 24)
    assert lib.mimo_coded_codewords(4096, 64, ctypes.byref(fits)) == 2
    # 39 rows: 2,048 + 159,744 + 96 = 161,888 fits; 40 rows: 165,984 does not
    s = np.stack([np.arange(40) % 512, (3 * np.arange(40) + 1) % 512], axis=1)
    assert lib.mimo_coded_codewords(4096, 64, ctypes.byref(_engine.LdpcCode(512, s[:39]))) == 24
    big = _engine.LdpcCode(512, s)
    assert lib.mimo_coded_codewords(4096, 64, ctypes.byref(big)) == -1
    msg = lib.mimo_last_error().decode()
    assert "165984" in msg and "163840" in msg and "LDS" in msg, msg
    chan = np.ones(1024, np.int8)
    app = np.zeros(1024, np.int16)
    assert lib.mimo_ldpc_decode(ctypes.byref(big), chan.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), 1,
                                app.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))) == -1
    assert "165984" in lib.mimo_last_error().decode()


def test_ldpc_decode_refuses_values_beyond_63_and_accepts_no_codewords():
    code = good_code()
    for bad in (64, -64, 127, -128):
        chan = np.ones((2, 96), np.int8)
        chan[1, 5] = bad
        with pytest.raises(_engine.EngineError, match=r"chan\[101\]"):
            _engine.ldpc_decode(code, chan)
    with pytest.raises(_engine.EngineError, match="n_cw"):
        _engine._check(_engine.lib().mimo_ldpc_decode(ctypes.byref(code), None, -1, None))
    out = _engine.ldpc_decode(code, np.zeros((0, 96), np.int8))   # n_cw = 0: MIMO_OK, nothing touched
    assert out.shape == (0, 96)
    assert _engine.lib().mimo_ldpc_decode(ctypes.byref(code), None, 0, None) == 0
    with pytest.raises(ValueError, match="whole codewords"):
        _engine.ldpc_decode(code, np.ones(95, np.int8))


def test_abi8_library_without_coded_is_reported_by_name(tmp_path, monkeypatch):
    """The coded entry points were added within ABI 8: a library that answers 8 and exports everything
    but them is reported as lacking a named entry point ('rebuild it')."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    mine = ("mimo_coded_width", "mimo_coded_codewords", "mimo_engine_coded_points", "mimo_engine_last_decode_ms",
            "mimo_ldpc_decode")
    assert all(n in _engine.SYMBOLS for n in mine)
    names = [n for n in _engine.SYMBOLS if n not in mine]
    src = tmp_path / "stale.c"
    src.write_text("int mimo_abi_version(void) { return 8; }\n" +
                   "".join(f"void {n}(void) {{}}\n" for n in names if n != "mimo_abi_version"))
    so = tmp_path / "libstale8.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(so))
    with pytest.raises(_engine.EngineError, match=r"\(ABI 8\) lacks mimo_coded_width: rebuild it"):
        _engine.lib()


# ---------------------------------------------------------------- qc_ldpc_code
def four_cycles(z, s):
    """Pairs of rows and columns of the shift table that close a cycle of length 4."""
    n_rows, n_cols = s.shape
    return [(r1, r2, c1, c2) for r1 in range(n_rows) for r2 in range(r1 + 1, n_rows) for c1 in range(n_cols)
            for c2 in range(c1 + 1, n_cols) if (int(s[r1, c1]) - int(s[r1, c2]) + int(s[r2, c2]) - int(s[r2, c1])) % z == 0]


@pytest.mark.parametrize("z,n_rows,n_cols", [(16, 3, 6), (61, 3, 6), (64, 4, 8), (128, 4, 8), (512, 12, 24), (512, 3, 6)])
def test_qc_ldpc_code_is_deterministic_full_and_free_of_4_cycles(z, n_rows, n_cols):
    a, b = qc_ldpc_code(z, n_rows, n_cols), qc_ldpc_code(z, n_rows, n_cols)
    assert (a.z, a.n_rows, a.n_cols, a.n_dec_iters) == (z, n_rows, n_cols, 10)
    np.testing.assert_array_equal(a.table, b.table)
    assert a.table.dtype == np.int16 and a.table.min() >= 0 and a.table.max() < z
    assert four_cycles(z, a.table) == []
    assert not np.array_equal(qc_ldpc_code(z, n_rows, n_cols, seed=1).table, a.table)
    assert qc_ldpc_code(z, n_rows, n_cols, n_dec_iters=3).n_dec_iters == 3
    # the draws of the text: the first column is the generator's first draw
    np.testing.assert_array_equal(a.table[:, 0], np.random.default_rng(0).integers(0, z, n_rows))
    # the structure points at the table the object keeps
    assert ctypes.addressof(a.shifts.contents) == a.table.ctypes.data


def test_qc_ldpc_code_gives_up_with_a_value_error():
    with pytest.raises(ValueError, match="column"):
        qc_ldpc_code(2, 3, 6)  # differences of 2 shifts take 2 values: a third column always repeats one


# ---------------------------------------------------------------- CodedStats
def test_coded_stats_arithmetic():
    cells = np.array([[10.0, 0.0, 0.0, 0.0], [262.0, 18.0, 2.0, 2.0], [300.0, 40.0, 3.0, 1.0]])
    st = _engine.CodedStats(cells, 48, 96)
    assert (st.n_idx, st.n_frames, st.n_code_bits, st.n_bits) == (3, 48, 96, 4608)
    np.testing.assert_array_equal(st.raw_ber(), cells[:, 0] / 4608)
    np.testing.assert_array_equal(st.ber(), cells[:, 1] / 4608)
    np.testing.assert_array_equal(st.fer(), cells[:, 2] / 48)
    np.testing.assert_array_equal(st.syndrome_rate(), cells[:, 3] / 48)
    np.testing.assert_array_equal(st.undetected(), (cells[:, 2] - cells[:, 3]) / 48)
    both = st + _engine.CodedStats(cells[::-1], 12, 96)
    assert both.n_frames == 60
    np.testing.assert_array_equal(both.cells, cells + cells[::-1])
    np.testing.assert_array_equal(both.fer(), (cells[:, 2] + cells[::-1, 2]) / 60)
    with pytest.raises(ValueError):
        st + _engine.CodedStats(cells, 48, 97)
    with pytest.raises(ValueError):
        st + _engine.CodedStats(cells[:2], 48, 96)
    empty = _engine.CodedStats(np.zeros((2, 4)), 0, 96)
    assert np.all(empty.ber() == 0) and np.all(empty.fer() == 0)
    flat = _engine.CodedStats(cells.reshape(-1), 48, 96)  # a flat row of n_idx * 4 cells
    np.testing.assert_array_equal(flat.cells, cells)
    assert "fer=" in repr(st)


# ---------------------------------------------------------------- the reference's own properties
def ref_code(z=16, n_rows=3, n_cols=6, n_dec_iters=10):
    return ldpc_ref.Code(z, qc_ldpc_code(z, n_rows, n_cols).table, n_dec_iters)


def parity_matrix(code):
    H = np.zeros((code.n_rows * code.z, code.n_bits), np.uint8)
    for r, idx in enumerate(code.layers()):
        for row in idx:
            H[r * code.z + np.arange(code.z), row] ^= 1
    return H


def nonzero_codeword(code):
    """A non-zero x with H x = 0 over GF(2), by elimination: the free column of lowest index set to 1."""
    H = parity_matrix(code).copy()
    n = H.shape[1]
    pivots, row = [], 0
    for col in range(n):
        hit = np.nonzero(H[row:, col])[0]
        if hit.size == 0:
            continue
        H[[row, row + hit[0]]] = H[[row + hit[0], row]]
        for other in np.nonzero(H[:, col])[0]:
            if other != row:
                H[other] ^= H[row]
        pivots.append(col)
        row += 1
        if row == H.shape[0]:
            break
    free = [c for c in range(n) if c not in pivots]
    x = np.zeros(n, np.uint8)
    x[free[0]] = 1
    for r, pc in enumerate(pivots):
        x[pc] = H[r, free[0]]
    return x


def test_reference_quantiser_and_stream():
    # scale 2: floor(rho * 2) clamped to [-32, 31], doubled, plus one
    rho = np.array([-1e9, -16.0, -15.9, -0.5, -0.4, 0.0, 0.49, 0.5, 15.49, 15.5, 1e9])
    np.testing.assert_array_equal(ldpc_ref.quantise(rho, 16.0),
                                  [-63, -63, -63, -1, -1, 1, 1, 3, 61, 63, 63])
    code = ref_code()
    chan = np.arange(2 * 96 + 5)  # a stream with 5 positions left over: bit n of codeword w at 2 n + w
    cw = ldpc_ref.codewords(code, chan)
    assert cw.shape == (2, 96)
    np.testing.assert_array_equal(cw[0], 2 * np.arange(96))
    np.testing.assert_array_equal(cw[1], 2 * np.arange(96) + 1)


def test_reference_keeps_a_clean_input_clean():
    code = ref_code()
    rng = np.random.default_rng(3)
    chan = 2 * rng.integers(0, 32, (5, 96)) + 1   # odd, positive
    cells, L = ldpc_ref.cells(code, chan)
    assert np.all(L > 0) and np.all(L >= chan)      # every message agrees with the bit
    np.testing.assert_array_equal(cells, [0, 0, 0, 0])
    assert not ldpc_ref.syndrome(code, L).any()


def test_reference_commutes_with_the_sign_flips_of_a_codeword():
    """decode(c (-1)^x) == decode(c) (-1)^x for a non-zero codeword x of the z 16, 3 x 6 code and random
    c in [-63, 63], zeros included: what lets the all-zero codeword stand for the scrambled link."""
    code = ref_code()
    x = nonzero_codeword(code)
    H = parity_matrix(code)
    assert x.any() and not ((H.astype(np.int64) @ x) & 1).any()
    rng = np.random.default_rng(5)
    c = rng.integers(-63, 64, (40, 96))
    c[:, ::7] = 0
    flip = 1 - 2 * x.astype(np.int64)
    for iters in (1, 10):
        cd = code.with_iters(iters)
        np.testing.assert_array_equal(ldpc_ref.decode(cd, c * flip), ldpc_ref.decode(cd, c) * flip)
    assert (ldpc_ref.decode(code, c) < 0).any() and x.sum() >= 2   # neither side of the identity is trivial


# ---------------------------------------------------------------- the sweep grid on a fake link
def test_coded_ber_vs_ebn0_and_csv_writer(tmp_path):
    import sweep
    from utilities import ebn0_to_snr, read_from_csv, save_to_csv
    link = fcl.FakeCodedLink()
    code = good_code()
    ibos, ebn0 = np.array([0.0, 4.0]), np.array([6.0, 10.0, 14.0])
    stats = sweep.coded_ber_vs_ebn0(link, ibos, ebn0, [0, 1], 5, code, seed=11)
    snr = [float(v) for v in ebn0_to_snr(ebn0, fcl.N_SC, fcl.N_SC, fcl.M)]
    assert len(link.calls) == 3  # the IBOs of one Eb/N0 in one call
    for j, call in enumerate(link.calls):
        assert call["ibos"] == [0.0, 4.0] and call["snrs"] == [snr[j]] * 2 and call["n_trials"] == 5
        assert call["iters"] == [0, 1] and call["incl_clean"] is False and call["reroll_chan"] is True
        assert call["rho_max"] is None and call["code"] is code
        assert call["seeds"] == [sweep.point_seed(11, i * 3 + j) for i in range(2)]
    assert len(stats) == 2 and all(len(r) == 3 for r in stats)
    for i, ibo in enumerate(ibos):
        for j in range(3):
            np.testing.assert_array_equal(stats[i][j].cells, fcl.fake_cells(ibo, snr[j], 5))
    sweep.coded_ber_vs_ebn0(link, ibos[:1], ebn0[:1], [0], 2, code, seed=11, incl_clean=True, reroll_chan=False,
                            rho_max=4.0)
    assert link.calls[3]["rho_max"] == 4.0 and link.calls[3]["incl_clean"] is True
    assert link.calls[3]["reroll_chan"] is False
    rows = sweep.coded_ber_vs_ebn0_rows(ebn0, stats[1])
    save_to_csv(rows, "coded", directory=str(tmp_path))
    back = np.asarray(read_from_csv("coded", directory=str(tmp_path)))
    assert back.shape == (1 + 4 * fcl.N_IDX, 3)
    np.testing.assert_array_equal(back[0], ebn0)
    frames = 5 * fcl.N_CW
    bits = frames * fcl.N_CODE_BITS
    for k in range(fcl.N_IDX):
        for j in range(3):
            c = fcl.fake_cells(4.0, snr[j], 5)[k]
            assert back[1 + 4 * k, j] == c[0] / bits and back[2 + 4 * k, j] == c[1] / bits
            assert back[3 + 4 * k, j] == c[2] / frames and back[4 + 4 * k, j] == c[3] / frames
