"""The C-ABI boundary on a machine without a GPU: the library loads, exports every entry
point include/mimo_engine.h declares, and validates configurations host-side with the
reference's error messages (no HIP call happens before the first compute call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mimo_engine.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mimo_\w+)\s*\(", text)))


def test_header_and_binding_agree():
    names = declared_functions()
    assert len(names) >= 20
    assert sorted(_engine.SYMBOLS) == names


def test_library_exports_every_declared_symbol():
    lib = _engine.lib()
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.mimo_abi_version() == 8


def test_build_entry_checks_the_header_abi():
    """__graft_entry__.build() compares the library's ABI with include/mimo_engine.h's
    MIMO_ABI_VERSION (a hard-coded number there went stale once: ABI 5 -> 6)."""
    import __graft_entry__ as g
    assert g._header_abi_version() == _engine.lib().mimo_abi_version() == 8


def _cfg(tx=None, fr=None, rx_pos=(0.0, 0.0, 0.0), table=None, **kw):
    """A config that mimo_engine_create accepts (every position at the origin: nothing here runs
    it) altered by ``kw``; ``tx`` [n_ant, 3], ``fr`` [n_fft], ``table`` [n_ant, n_fft] complex
    replace the arrays, the string "null" passes a null pointer."""
    dp = ctypes.POINTER(ctypes.c_double)
    if tx is None:
        tx = np.zeros((kw.get("n_ant", 4), 3))
    if fr is None:
        fr = np.full(kw.get("n_fft", 256), 3.5e9)
    keep = [None if a is None or isinstance(a, str) else np.ascontiguousarray(a, dtype=t)
            for a, t in ((tx, np.float64), (fr, np.float64), (table, np.complex128))]
    ptr = [None if a is None else a.view(np.float64).ctypes.data_as(dp) for a in keep]
    base = dict(n_ant=4, n_sub_carr=128, n_fft=256, constel_size=16, cp_len=16, channel_kind=1, receiver_kind=1,
                device=-1, rx_loc_var=10.0, reroll_chan=1, precision=0)
    base.update(kw)
    c = _engine.MimoConfig(**base, tx_pos=ptr[0], carrier_freqs=ptr[1], chan_table=ptr[2])
    c.rx_pos[:] = [float(v) for v in rx_pos]
    return c, keep


@pytest.mark.parametrize("kw,msg", [
    (dict(n_fft=300), "n_fft must be a power of two"),
    (dict(n_fft=16384), "n_fft must be a power of two"),
    (dict(n_sub_carr=256), "n_sub_carr must be a multiple of 4"),
    (dict(n_sub_carr=126), "n_sub_carr must be a multiple of 4"),
    (dict(constel_size=8), "only square QAM supported"),      # modulation.py:236-237
    (dict(constel_size=36), "only square QAM supported"),
    (dict(n_ant=0), "n_ant must be in"),
    (dict(channel_kind=7), "unknown channel_kind"),
    (dict(receiver_kind=0), "unknown receiver_kind"),
    (dict(precision=2), "precision must be"),
    (dict(chan_replay_period=-1), "chan_replay_period must be >= 0"),
    (dict(chan_replay_period=8, channel_kind=2), "Rayleigh channel only"),
])
def test_create_rejects_invalid_configs(kw, msg):
    lib = _engine.lib()
    c, keep = _cfg(**kw)
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert not h
    assert msg in lib.mimo_last_error().decode()


NAN, INF = float("nan"), float("inf")


def _geo(**kw):
    """_cfg on a geometry that can run: antennas 1 m apart on a line 15 m up (_line), the default user."""
    kw.setdefault("tx", _line())
    kw.setdefault("rx_pos", (212.0, 212.0, 1.5))
    return _cfg(**kw)


def _line(n_ant=4, **cells):
    """_geo's antennas with single coordinates replaced: a1y=NAN sets antenna 1's y."""
    tx = np.stack([np.arange(n_ant, dtype=np.float64), np.zeros(n_ant), np.full(n_ant, 15.0)], axis=1)
    for key, v in cells.items():
        tx[int(key[1:-1]), "xyz".index(key[-1])] = v
    return tx


def _freqs(n_fft=256, **bins):
    """_cfg's carriers with single bins replaced: b5=0.0 sets bin 5."""
    fr = np.full(n_fft, 3.5e9)
    for key, v in bins.items():
        fr[int(key[1:])] = v
    return fr


def _table(n_ant=4, n_fft=256, **cells):
    """A finite channel table with single entries replaced: a3k255=NAN sets antenna 3, bin 255."""
    tab = np.full((n_ant, n_fft), 0.5 - 0.25j)
    for key, v in cells.items():
        a, k = key[1:].split("k")
        tab[int(a), int(k)] = v
    return tab


RAYLEIGH, LOS, TWOPATH, TABLE = 1, 2, 3, 4
GEOMETRY_REJECTS = {
    # tx_pos: all 3 n_ant values finite -- each coordinate, the first and the last antenna
    "tx_nan_first_x": (dict(tx=_line(a0x=NAN)), "tx_pos must be finite"),
    "tx_inf_y": (dict(tx=_line(a1y=INF)), "tx_pos must be finite"),
    "tx_minus_inf_last_z": (dict(tx=_line(a3z=-INF)), "tx_pos must be finite"),
    "tx_nan_table_channel": (dict(tx=_line(a2z=NAN), channel_kind=TABLE, table=_table()), "tx_pos must be finite"),
    # rx_pos: finite, each coordinate
    "rx_nan_x": (dict(rx_pos=(NAN, 212.0, 1.5)), "rx_pos must be finite"),
    "rx_inf_y": (dict(rx_pos=(212.0, INF, 1.5)), "rx_pos must be finite"),
    "rx_minus_inf_z": (dict(rx_pos=(212.0, 212.0, -INF)), "rx_pos must be finite"),
    "rx_nan_los": (dict(rx_pos=(NAN, 212.0, 1.5), channel_kind=LOS), "rx_pos must be finite"),
    # rx_loc_var: finite and >= 0
    "var_nan": (dict(rx_loc_var=NAN), "rx_loc_var must be finite and >= 0"),
    "var_inf": (dict(rx_loc_var=INF), "rx_loc_var must be finite and >= 0"),
    "var_minus_inf": (dict(rx_loc_var=-INF), "rx_loc_var must be finite and >= 0"),
    "var_negative": (dict(rx_loc_var=-10.0, channel_kind=LOS), "rx_loc_var must be finite and >= 0"),
    # carrier_freqs: required, all n_fft values finite and > 0
    "freqs_null": (dict(fr="null"), "carrier_freqs is required"),
    "freq_nan_centre": (dict(fr=_freqs(b0=NAN)), "carrier_freqs must be finite and > 0"),
    "freq_inf": (dict(fr=_freqs(b7=INF)), "carrier_freqs must be finite and > 0"),
    "freq_minus_inf": (dict(fr=_freqs(b128=-INF)), "carrier_freqs must be finite and > 0"),
    "freq_zero_last_bin": (dict(fr=_freqs(b255=0.0)), "carrier_freqs must be finite and > 0"),
    "freq_negative": (dict(fr=_freqs(b200=-3.5e9)), "carrier_freqs must be finite and > 0"),
    "freq_zero_out_of_band": (dict(fr=_freqs(b128=0.0)), "carrier_freqs must be finite and > 0"),
    # TABLE: every entry finite
    "table_nan_real": (dict(channel_kind=TABLE, table=_table(a0k0=NAN)), "chan_table must be finite"),
    "table_inf_imag_last": (dict(channel_kind=TABLE, table=_table(a3k255=complex(0.0, INF))), "chan_table must be finite"),
    "table_minus_inf_out_of_band": (dict(channel_kind=TABLE, table=_table(a1k128=-INF)), "chan_table must be finite"),
}
# the rule every run call checks: the distances the channel divides by
DISTANCE_REJECTS = {
    # every channel but TABLE: no antenna at rx_pos
    "user_on_antenna_rayleigh": (dict(rx_pos=(2.0, 0.0, 15.0)), "rx_pos is no finite distance > 0 from antenna 2"),
    "user_on_antenna_los": (dict(rx_pos=(3.0, 0.0, 15.0), channel_kind=LOS),
                            "rx_pos is no finite distance > 0 from antenna 3"),
    "user_on_antenna_two_path": (dict(rx_pos=(0.0, 0.0, 15.0), channel_kind=TWOPATH),
                                 "rx_pos is no finite distance > 0 from antenna 0"),
    # ... nor so close that the distance rounds to 0 (the square of 1e-170 underflows)
    "user_at_rounding_distance": (dict(rx_pos=(1e-170, 0.0, 15.0)), "rx_pos is no finite distance > 0 from antenna 0"),
    # ... nor so far that it overflows
    "user_beyond_overflow": (dict(rx_pos=(1e200, 0.0, 15.0)), "rx_pos is no finite distance > 0 from antenna 0"),
    # LoS and two-path also: no antenna at (rx_pos[0], rx_pos[0], rx_pos[2]), the jitter's centre
    "jitter_centre_on_antenna_los": (dict(rx_pos=(5.0, 9.0, 15.0), tx=_line(a1x=5.0, a1y=5.0), channel_kind=LOS),
                                     "rx_pos: the jitter's centre"),
    "jitter_centre_on_antenna_two_path": (dict(rx_pos=(5.0, 9.0, 15.0), tx=_line(a3x=5.0, a3y=5.0),
                                               channel_kind=TWOPATH), "rx_pos: the jitter's centre"),
    # what the host tests of earlier rounds build: every antenna and the user at the origin
    "everything_at_the_origin": (dict(tx=np.zeros((4, 3)), rx_pos=(0.0, 0.0, 0.0)),
                                 "rx_pos is no finite distance > 0 from antenna 0"),
}


@pytest.mark.parametrize("name", sorted(GEOMETRY_REJECTS))
def test_create_rejects_a_broken_geometry_by_field(name):
    """The geometry rules of mimo_config (include/mimo_engine.h): a NaN or infinite coordinate, a
    negative or non-finite jitter span, a carrier frequency that is missing, 0, negative or not
    finite, a non-finite table entry -- each used to reach the kernel and come back as
    ordinary-looking counts.  Now a null engine and a message that starts with the field; all
    host-side, no HIP call."""
    lib = _engine.lib()
    kw, msg = GEOMETRY_REJECTS[name]
    c, keep = _geo(**kw)
    h = lib.mimo_engine_create(ctypes.byref(c))
    if h:
        lib.mimo_engine_destroy(h)
    assert not h, f"{name}: accepted"
    assert lib.mimo_last_error().decode().startswith(msg), lib.mimo_last_error()


@pytest.mark.parametrize("kw", [
    dict(rx_loc_var=0.0),                                              # a fixed user
    dict(rx_loc_var=0.0, channel_kind=LOS),
    dict(rx_pos=(-212.0, -212.0, -1.5), tx=_line(a0x=-3.0, a0z=-15.0)),  # negative coordinates
    dict(fr=_freqs(b0=1.0, b255=5e-324)),                              # any frequency > 0
])
def test_create_keeps_every_legitimate_geometry(kw):
    lib = _engine.lib()
    c, keep = _geo(**kw)
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h, lib.mimo_last_error()
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("name", sorted(DISTANCE_REJECTS))
def test_run_refuses_an_antenna_at_the_user_before_any_hip_call(name):
    """A user standing on an antenna (the attenuation's distance 0: ant_rel = inf), at a distance
    that rounds to 0 or overflows, or, for LoS / two-path, an antenna at the centre the jitter is
    really drawn around, used to run and come back as ordinary-looking counts.  The engine can be
    created, described and given a point as before -- no run, no division -- and
    mimo_engine_run and mimo_engine_run_points are MIMO_EINVAL with a message that starts with the
    field, host-side: on a machine without a GPU a HIP call would be MIMO_EHIP instead."""
    lib = _engine.lib()
    kw, msg = DISTANCE_REJECTS[name]
    c, keep = _geo(**kw)
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h, lib.mimo_last_error()
    good = _engine.Engine.make_point(**GOOD_POINT)
    assert lib.mimo_engine_set_point(h, ctypes.byref(good)) == 0
    assert lib.mimo_engine_describe(h).decode().startswith("F=256")
    it = np.zeros(1, np.int32)
    err, bits = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_run(h, 1, 0, 4, it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 0,
                             err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None)
    assert rc == -1 and not err.any() and not bits.any()  # MIMO_EINVAL
    assert lib.mimo_last_error().decode().startswith(msg), lib.mimo_last_error()
    assert _run_points_rc(lib, h, [good, good]) == -1
    assert lib.mimo_last_error().decode().startswith(msg), lib.mimo_last_error()
    lib.mimo_engine_destroy(h)


def test_engine_class_surfaces_the_geometry_message():
    """_engine.Engine raises the library's message, as for the other config errors: ValueError
    from the constructor, EngineError from run and from the measure, spectrum and beam modes."""
    good = dict(n_ant=4, n_sub_carr=128, n_fft=256, constel_size=16, cp_len=16, channel="los", receiver="cnc",
                tx_pos=_line(), rx_pos=(212.0, 212.0, 1.5), rx_loc_var=10.0, carrier_freqs=_freqs())
    _engine.Engine(**good).close()
    for change, msg in ((dict(carrier_freqs=_freqs(b9=0.0)), "carrier_freqs must be finite and > 0 \\(bin 9\\)"),
                        (dict(tx_pos=_line(a2z=NAN)), "tx_pos must be finite \\(antenna 2\\)"),
                        (dict(rx_loc_var=-1.0), "rx_loc_var must be finite and >= 0"),
                        (dict(channel="table", chan_table=_table(a1k3=NAN)), "chan_table must be finite \\(antenna 1\\)")):
        with pytest.raises(ValueError, match=msg):
            _engine.Engine(**dict(good, **change))
    eng = _engine.Engine(**dict(good, rx_pos=(1.0, 1.0, 15.0), tx_pos=_line(a1y=1.0)))
    eng.set_point(**GOOD_POINT)
    msg = "rx_pos is no finite distance > 0 from antenna 1"
    probes = np.array([[212.0, 212.0, 1.5]])
    for call in (lambda: eng.run(1, 0, 4, [0]), lambda: eng.measure(1, 0, 4, [0]), lambda: eng.spectrum(1, 0, 4, [0]),
                 lambda: eng.beam(1, 0, 4, [0], probes)):
        with pytest.raises(_engine.EngineError, match=msg):
            call()
    eng.close()


def test_valid_engine_is_host_only_until_run():
    """create / set_point / describe / destroy never touch HIP (fork safety)."""
    lib = _engine.lib()
    c, keep = _cfg(n_fft=512, n_sub_carr=256)
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h
    pt = _engine.MimoPoint(ibo_db=3.0, snr_db=20.0, avg_symbol_power=10.0, pa_kind=1, cnc_pa_kind=1, sat_pow=1.0,
                           p_hardness=0.0, toi_coeff=0.0, cnc_sat_pow=1.0, cnc_toi_coeff=0.0, cnc_alpha=0.9,
                           csi_eps=-1.0)
    assert lib.mimo_engine_set_point(h, ctypes.byref(pt)) == 0
    desc = lib.mimo_engine_describe(h).decode()
    assert "F=512" in desc and "aligned" in desc and desc.endswith("f64"), desc
    bad = _engine.MimoPoint(**{f: getattr(pt, f) for f, _ in _engine.MimoPoint._fields_})
    bad.csi_eps = 1.5
    assert lib.mimo_engine_set_point(h, ctypes.byref(bad)) == -1  # MIMO_EINVAL
    assert "csi_eps" in lib.mimo_last_error().decode()
    lib.mimo_engine_destroy(h)


def test_set_point_array_alpha_validation():
    """mimo_point.array_alpha (ABI 8): 0 = per-antenna gains; > 0 accepted by the float64
    instances and by float32 up to F 4096; negative / non-finite values and float32 F 8192
    (no alpha polynomial in that instance) are MIMO_EINVAL -- all host-side, no HIP."""
    lib = _engine.lib()
    for prec, n_fft, alpha, ok in ((0, 512, 0.93, True), (1, 512, 0.93, True), (0, 8192, 0.93, True),
                                   (1, 8192, 0.93, False), (1, 8192, 0.0, True), (0, 512, -0.5, False),
                                   (0, 512, float("nan"), False), (0, 512, float("inf"), False)):
        c, keep = _cfg(n_fft=n_fft, n_sub_carr=n_fft // 2, precision=prec)
        h = lib.mimo_engine_create(ctypes.byref(c))
        assert h
        pt = _engine.Engine.make_point(3.0, 20.0, 10.0, "toi", toi_coeff=0.01, cnc_toi_coeff=0.01, cnc_alpha=0.9,
                                       array_alpha=alpha)
        rc = lib.mimo_engine_set_point(h, ctypes.byref(pt))
        assert (rc == 0) == ok, (prec, n_fft, alpha, rc, lib.mimo_last_error())
        if not ok:
            assert "array_alpha" in lib.mimo_last_error().decode()
        lib.mimo_engine_destroy(h)


NAN, INF = float("nan"), float("inf")
# a valid soft-limiter / soft-limiter point (make_point keywords), which every case below alters
GOOD_POINT = dict(ibo_db=3.0, snr_db=20.0, avg_symbol_power=10.0, pa_kind="softlim", sat_pow=1.0, cnc_sat_pow=1.0,
                  cnc_alpha=0.9)


def _run_points_rc(lib, h, pts):
    """mimo_engine_run_points over ``pts`` (MimoPoint), 4 trials each, iteration 0."""
    n = len(pts)
    arr = (_engine.MimoPoint * n)(*pts)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    seeds, first, ntr = np.arange(1, n + 1, dtype=np.uint64), np.zeros(n, np.uint64), np.full(n, 4, np.uint64)
    it = np.zeros(1, np.int32)
    err, bits = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    rc = lib.mimo_engine_run_points(h, n, arr, seeds.ctypes.data_as(u64), first.ctypes.data_as(u64),
                                    ntr.ctypes.data_as(u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 0,
                                    err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None)
    assert not err.any() and not bits.any()
    return rc


@pytest.mark.parametrize("receiver,change,field", [
    # the receiver's saturation power where its soft limiter / Rapp model divides by it
    ("cnc", dict(cnc_sat_pow=0.0), "cnc_sat_pow"),
    ("cnc", dict(cnc_sat_pow=-1.0), "cnc_sat_pow"),
    ("cnc", dict(cnc_sat_pow=NAN), "cnc_sat_pow"),
    ("cnc", dict(cnc_pa_kind="rapp", p_hardness=3.0, cnc_sat_pow=0.0), "cnc_sat_pow"),
    ("cnc", dict(cnc_pa_kind="rapp", p_hardness=3.0, cnc_sat_pow=NAN), "cnc_sat_pow"),
    ("cnc", dict(pa_kind="toi", toi_coeff=0.01, sat_pow=0.0, cnc_pa_kind="softlim", cnc_sat_pow=0.0), "cnc_sat_pow"),
    # the one Rapp hardness, read by a Rapp receiver under any array
    ("cnc", dict(cnc_pa_kind="rapp", p_hardness=0.0), "p_hardness"),
    ("cnc", dict(pa_kind="rapp", cnc_pa_kind="rapp", p_hardness=NAN), "p_hardness"),
    ("cnc", dict(cnc_alpha=NAN), "cnc_alpha"),
    ("mcnc", dict(cnc_alpha=NAN), "cnc_alpha"),
    ("cnc", dict(cnc_alpha=0.0), "cnc_alpha"),
    ("cnc", dict(snr_db=NAN), "snr_db"),
    ("cnc", dict(snr_db=INF), "snr_db"),
    ("cnc", dict(snr_db=-INF), "snr_db"),
    ("cnc", dict(snr_db=-4000.0), "snr_db"),  # 10^-400 underflows: an infinite noise power
    ("mcnc", dict(snr_db=NAN), "snr_db"),
    ("cnc", dict(ibo_db=NAN), "ibo_db"),
    ("cnc", dict(ibo_db=INF), "ibo_db"),
    ("cnc", dict(avg_symbol_power=NAN), "avg_symbol_power"),
    ("cnc", dict(avg_symbol_power=INF), "avg_symbol_power"),
    ("cnc", dict(avg_symbol_power=0.0), "avg_symbol_power"),
    ("cnc", dict(avg_symbol_power=-10.0), "avg_symbol_power"),
    ("cnc", dict(pa_kind="toi", cnc_pa_kind="toi", toi_coeff=NAN, cnc_toi_coeff=0.01), "toi_coeff"),
    ("cnc", dict(pa_kind="toi", cnc_pa_kind="toi", toi_coeff=INF, cnc_toi_coeff=0.01), "toi_coeff"),
    ("cnc", dict(pa_kind="toi", cnc_pa_kind="toi", toi_coeff=0.01, cnc_toi_coeff=NAN), "cnc_toi_coeff"),
    ("cnc", dict(cnc_pa_kind="toi", cnc_toi_coeff=-INF), "cnc_toi_coeff"),
    ("mcnc", dict(pa_kind="toi", cnc_pa_kind="toi", toi_coeff=NAN), "toi_coeff"),
    ("cnc", dict(csi_eps=NAN), "csi_eps"),
    ("mcnc", dict(csi_eps=NAN), "csi_eps"),
    ("cnc", dict(sat_pow=NAN), "sat_pow"),
    ("cnc", dict(sat_pow=0.0), "sat_pow"),
])
def test_point_validation_refuses_bad_fields_by_name(receiver, change, field):
    """A point whose field would run as something else -- a zero or NaN saturation power of the CNC
    receiver's PA (soft limiter: the re-synthesised signal scaled to 0; Rapp: the identity), a NaN
    alpha, SNR, IBO, symbol power or cubic coefficient, a NaN csi_eps (read as perfect CSI) -- is
    MIMO_EINVAL from mimo_engine_set_point and from mimo_engine_run_points, as the first point or
    after a valid one; the message names the field; all host-side, no HIP call."""
    lib = _engine.lib()
    c, keep = _cfg(n_fft=512, n_sub_carr=256, receiver_kind=_engine.RX_KINDS[receiver])
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h
    good = _engine.Engine.make_point(**GOOD_POINT)
    assert lib.mimo_engine_set_point(h, ctypes.byref(good)) == 0
    bad = _engine.Engine.make_point(**dict(GOOD_POINT, **change))
    assert lib.mimo_engine_set_point(h, ctypes.byref(bad)) == -1
    msg = lib.mimo_last_error().decode()
    assert msg.startswith(field), msg
    for pts in ([bad], [good, bad]):
        assert _run_points_rc(lib, h, pts) == -1
        assert lib.mimo_last_error().decode() == msg
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("receiver,change", [
    ("cnc", dict(pa_kind="toi", cnc_pa_kind="toi", sat_pow=0.0, cnc_sat_pow=0.0, toi_coeff=0.01, cnc_toi_coeff=0.01)),
    ("cnc", dict(pa_kind="none", cnc_pa_kind="none", sat_pow=0.0, cnc_sat_pow=0.0)),
    ("cnc", dict(cnc_pa_kind="none", cnc_sat_pow=0.0)),
    ("cnc", dict(cnc_pa_kind="toi", cnc_sat_pow=0.0, cnc_toi_coeff=0.01)),
    ("mcnc", dict(cnc_sat_pow=0.0)),                      # MCNC reads no cnc_* field
    ("mcnc", dict(cnc_pa_kind="rapp", cnc_sat_pow=0.0, p_hardness=0.0)),
    ("mcnc", dict(cnc_pa_kind="toi", cnc_toi_coeff=NAN)),
    ("cnc", dict(sat_pow=INF)),                           # an array PA that never saturates
    ("cnc", dict(cnc_sat_pow=INF)),
    ("cnc", dict(csi_eps=0.0)),
    ("cnc", dict(csi_eps=-1.0)),
    ("cnc", dict(snr_db=1000.0)),                         # noiseless
    ("cnc", dict(snr_db=-50.0)),
    ("cnc", dict(toi_coeff=NAN)),                         # not read: the array is a soft limiter
    ("cnc", dict(cnc_toi_coeff=NAN)),
    ("cnc", dict(pa_kind="rapp", cnc_pa_kind="softlim", p_hardness=2.5)),   # the receiver's model differs
    ("cnc", dict(pa_kind="softlim", cnc_pa_kind="rapp", p_hardness=2.5)),
])
def test_point_validation_keeps_every_legitimate_edge(receiver, change):
    """The edges that stay valid: a zero saturation power where no soft limiter / Rapp reads it (the
    TOI drivers' points, any cnc_* field under MCNC), an infinite one, csi_eps = 0, a noiseless SNR,
    a receiver PA of another kind than the array's."""
    lib = _engine.lib()
    c, keep = _cfg(n_fft=512, n_sub_carr=256, receiver_kind=_engine.RX_KINDS[receiver])
    h = lib.mimo_engine_create(ctypes.byref(c))
    pt = _engine.Engine.make_point(**dict(GOOD_POINT, **change))
    assert lib.mimo_engine_set_point(h, ctypes.byref(pt)) == 0, lib.mimo_last_error()
    lib.mimo_engine_destroy(h)


def test_published_toi_points_pass_the_point_validation():
    """tools/published_families sends sat_pow = cnc_sat_pow = 0 with its TOI points: still valid."""
    import published_families as pf
    lib = _engine.lib()
    first = {}  # the first TOI curve of each receiver kind
    for curve in pf.CURVES:
        if curve["family"] == "toi":
            first.setdefault(curve["receiver"], curve)
    assert "cnc" in first
    for receiver, curve in first.items():
        c, keep = _cfg(n_fft=512, n_sub_carr=256, receiver_kind=_engine.RX_KINDS[receiver])
        h = lib.mimo_engine_create(ctypes.byref(c))
        _, pts = pf.points(dict(curve), np.array([10.0, 15.0]))
        for pp in pts:
            assert pp["sat_pow"] == 0.0 and pp["cnc_sat_pow"] == 0.0
            pt = _engine.Engine.make_point(**pp)
            assert lib.mimo_engine_set_point(h, ctypes.byref(pt)) == 0, (curve, lib.mimo_last_error())
        lib.mimo_engine_destroy(h)


def test_run_points_refuses_a_mix_of_csi_on_and_off():
    """All points of one call run one kernel instance, with or without the CSI error model: a call
    whose points disagree is MIMO_EINVAL before any HIP call, whichever comes first."""
    lib = _engine.lib()
    c, keep = _cfg(n_fft=512, n_sub_carr=256)
    h = lib.mimo_engine_create(ctypes.byref(c))
    off = _engine.Engine.make_point(**GOOD_POINT)
    for eps in (0.0, 0.2):
        on = _engine.Engine.make_point(**dict(GOOD_POINT, csi_eps=eps))
        for pts in ([off, on], [on, off], [on, on, off]):
            assert _run_points_rc(lib, h, pts) == -1
            assert "agree on CSI" in lib.mimo_last_error().decode()
    lib.mimo_engine_destroy(h)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_engine.EngineError, match="not found"):
        _engine.lib()


def _engine_with_point():
    lib = _engine.lib()
    c, keep = _cfg(n_fft=512, n_sub_carr=256)
    h = lib.mimo_engine_create(ctypes.byref(c))
    pt = _engine.MimoPoint(ibo_db=3.0, snr_db=20.0, avg_symbol_power=10.0, pa_kind=1, cnc_pa_kind=1, sat_pow=1.0,
                           p_hardness=0.0, toi_coeff=0.0, cnc_sat_pow=1.0, cnc_toi_coeff=0.0, cnc_alpha=0.9,
                           csi_eps=-1.0)
    assert lib.mimo_engine_set_point(h, ctypes.byref(pt)) == 0
    return lib, h, pt, keep


@pytest.mark.parametrize("iters,first,n,msg", [
    ([2, 1], 0, 8, "sorted and unique"),
    ([1, 1], 0, 8, "sorted and unique"),
    ([32], 0, 8, "[0, 31]"),
    ([-1], 0, 8, "[0, 31]"),
    ([], 0, 8, "at least one iteration"),
    ([0], (1 << 32) - 4, 8, "fit 32 bits"),
])
def test_run_validates_arguments_before_any_hip_call(iters, first, n, msg):
    lib, h, pt, keep = _engine_with_point()
    it = np.asarray(iters, np.int32)
    err = np.zeros(4, np.uint64)
    bits = np.zeros(4, np.uint64)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    rc = lib.mimo_engine_run(h, 1, first, n, it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(it), 0,
                             err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None)
    assert rc == -1 and msg in lib.mimo_last_error().decode()
    # before set_point
    c, keep2 = _cfg(n_fft=512, n_sub_carr=256)
    h2 = lib.mimo_engine_create(ctypes.byref(c))
    it0 = np.zeros(1, np.int32)
    rc = lib.mimo_engine_run(h2, 1, 0, 8, it0.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 0,
                             err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None)
    assert rc == -1 and "set_point" in lib.mimo_last_error().decode()
    lib.mimo_engine_destroy(h)
    lib.mimo_engine_destroy(h2)


@pytest.mark.parametrize("prec,team", [(0, 64), (1, 64)])
def test_precision_selects_the_instance(prec, team):
    """precision = MIMO_PREC_F64 (default 0: the reference's float64) or MIMO_PREC_F32."""
    lib = _engine.lib()
    c, keep = _cfg(n_fft=2048, n_sub_carr=1024, precision=prec)
    h = lib.mimo_engine_create(ctypes.byref(c))
    desc = lib.mimo_engine_describe(h).decode()
    # fp64 teams hold 8 points per thread (T = F/8), fp32 teams 16 (T = F/16)
    assert desc.startswith("F=2048 T=256" if prec == 0 else "F=2048 T=128"), desc
    assert desc.endswith("f64" if prec == 0 else "f32"), desc
    lib.mimo_engine_destroy(h)


def test_calc_alpha_validates_without_a_gpu():
    """mimo_calc_alpha (ABI 6): an empty request succeeds and a negative count is rejected
    host-side, before any HIP call."""
    lib = _engine.lib()
    out = np.zeros(1)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.mimo_calc_alpha(out.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == 0
    assert lib.mimo_calc_alpha(out.ctypes.data_as(dp), -1, out.ctypes.data_as(dp)) == -1  # MIMO_EINVAL
    assert "n < 0" in lib.mimo_last_error().decode()


def test_stale_library_reports_its_abi(tmp_path, monkeypatch):
    """a library of an older ABI (here 6, without mimo_cnc_receive_ex) is reported
    as such -- the version is checked before the newer entry points are bound, so the error
    is the 'rebuild it' EngineError, not a bare AttributeError."""
    import shutil
    import subprocess
    import _engine
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "stale.c"
    src.write_text("int mimo_abi_version(void) { return 6; }\n")
    so = tmp_path / "libstale.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(so))
    with pytest.raises(_engine.EngineError, match="is ABI 6, this module ABI 8: rebuild it"):
        _engine.lib()


@pytest.mark.parametrize("n_fft,batch,msg", [(0, 1, "n_fft"), (-8, 1, "n_fft"), (3, 1, "n_fft"), (16384, 1, "n_fft"),
                                             (64, -1, "batch")])
def test_fft_validates_sizes_before_any_allocation(n_fft, batch, msg):
    """mimo_fft: n_fft <= 0, not a power of two or beyond 8192, and batch < 0 are MIMO_EINVAL,
    decided before the device buffers (whose size multiplies the two) are allocated: host only."""
    lib = _engine.lib()
    buf = np.zeros(4)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.mimo_fft(n_fft, batch, 0, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp)) == -1  # MIMO_EINVAL
    assert msg in lib.mimo_last_error().decode()


_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


def _seam_call(name, *args):
    """Call a fine seam with dummy 8-element buffers for every pointer argument: the calls
    below are all decided before the library looks at (or allocates for) any of them."""
    lib = _engine.lib()
    keep = []

    def buf(ptr_type, dtype):
        a = np.zeros(8, dtype)
        keep.append(a)
        return a.ctypes.data_as(ptr_type)

    d, i32, i64 = (lambda: buf(_dp, np.float64)), (lambda: buf(_i32p, np.int32)), (lambda: buf(_i64p, np.int64))
    if name == "mimo_qam_map":
        M, n = args
        return lib.mimo_qam_map(M, i32(), n, d())
    if name == "mimo_qam_slice":
        M, n = args
        return lib.mimo_qam_slice(M, d(), n, i32())
    if name == "mimo_qam_llr":
        M, n = args
        return lib.mimo_qam_llr(M, d(), n, d(), d())
    if name == "mimo_fft":
        F, batch = args
        return lib.mimo_fft(F, batch, 0, d(), d())
    if name in ("mimo_ofdm_tx", "mimo_ofdm_rx"):
        F, S, cp, batch = args
        return getattr(lib, name)(F, S, cp, batch, d(), d())
    if name == "mimo_pa":
        kind, n = args
        return lib.mimo_pa(kind, 1.0, 2.0, 0.1, d(), n, d())
    if name == "mimo_mrt_precode":
        A, K = args
        return lib.mimo_mrt_precode(A, K, d(), d())
    if name == "mimo_combine":
        A, K = args
        return lib.mimo_combine(A, K, d(), d(), d())
    if name == "mimo_awgn":
        (n,) = args
        return lib.mimo_awgn(1, 0, n, 1.0, d(), d())
    if name == "mimo_count_bit_errors":
        (n,) = args
        out = np.full(1, -7, np.int64)
        rc = lib.mimo_count_bit_errors(i64(), i64(), n, out.ctypes.data_as(_i64p))
        return rc if rc or n else (rc, int(out[0]))
    if name in ("mimo_cnc_receive", "mimo_cnc_receive_ex"):
        M, F, S, kind, alpha = args
        it = np.zeros(1, np.int32)
        tail = (i32(), d()) if name.endswith("_ex") else (i32(),)
        return getattr(lib, name)(M, F, S, kind, 1.0, 2.0, 0.1, alpha, it.ctypes.data_as(_i32p), 1, d(), *tail)
    raise KeyError(name)


_OFDM_REJECTS = [((128, 64, 4, -1), "batch must be >= 0"),
                 ((0, 64, 4, 1), "n_fft must be a power of two"),
                 ((-128, 64, 4, 1), "n_fft must be a power of two"),
                 ((96, 64, 4, 1), "n_fft must be a power of two"),
                 ((1, 2, 0, 1), "n_fft must be a power of two"),
                 ((16384, 64, 4, 1), "n_fft must be a power of two"),
                 ((128, 63, 4, 1), "n_sub_carr must be even"),
                 ((128, 0, 4, 1), "n_sub_carr must be even"),
                 ((128, -2, 4, 1), "n_sub_carr must be even"),
                 ((128, 128, 4, 1), "n_sub_carr must be even"),
                 ((2, 2, 0, 1), "n_sub_carr must be even"),
                 ((128, 64, -1, 1), "cp_len must be in [0, n_fft]"),
                 ((128, 64, 129, 1), "cp_len must be in [0, n_fft]")]
_CNC_REJECTS = [((16, 0, 64, 1, 0.9), "n_fft must be a power of two"),
                ((16, 100, 64, 1, 0.9), "n_fft must be a power of two"),
                ((16, 16384, 64, 1, 0.9), "n_fft must be a power of two"),
                ((16, 128, 63, 1, 0.9), "n_sub_carr must be even"),
                ((16, 128, 0, 1, 0.9), "n_sub_carr must be even"),
                ((16, 128, -4, 1, 0.9), "n_sub_carr must be even"),
                ((16, 128, 128, 1, 0.9), "n_sub_carr must be even"),
                ((16, 128, 64, -1, 0.9), "unknown PA kind"),
                ((16, 128, 64, 4, 0.9), "unknown PA kind"),
                ((16, 128, 64, 1, 0.0), "alpha must be finite and non-zero"),
                ((16, 128, 64, 1, float("nan")), "alpha must be finite and non-zero"),
                ((16, 128, 64, 1, float("inf")), "alpha must be finite and non-zero"),
                ((8, 128, 64, 1, 0.9), "only square QAM supported")]


@pytest.mark.parametrize("name,args,msg", [
    ("mimo_qam_map", (16, -1), "n must be >= 0"),
    ("mimo_qam_slice", (16, -1), "n must be >= 0"),
    ("mimo_qam_llr", (16, -1), "n must be >= 0"),
    ("mimo_qam_map", (8192, 4), "only square QAM supported"),
    ("mimo_pa", (1, -1), "n must be >= 0"),
    ("mimo_pa", (4, 4), "unknown PA kind"),
    ("mimo_awgn", (-1,), "n must be >= 0"),
    ("mimo_count_bit_errors", (-1,), "n must be >= 0"),
    ("mimo_count_bit_errors", (-(1 << 62),), "n must be >= 0"),
    ("mimo_mrt_precode", (0, 4), "n_ant must be >= 1"),
    ("mimo_mrt_precode", (-3, 4), "n_ant must be >= 1"),
    ("mimo_mrt_precode", (4, -1), "n_cols must be >= 0"),
    ("mimo_combine", (0, 4), "n_ant must be >= 1"),
    ("mimo_combine", (4, -1), "n must be >= 0"),
] + [(f, a, m) for f in ("mimo_ofdm_tx", "mimo_ofdm_rx") for a, m in _OFDM_REJECTS]
  + [(f, a, m) for f in ("mimo_cnc_receive", "mimo_cnc_receive_ex") for a, m in _CNC_REJECTS])
def test_fine_seams_reject_bad_sizes_before_any_hip_call(name, args, msg):
    """Every fine seam refuses a negative size, an n_fft / n_sub_carr / cp_len outside the
    ranges of include/mimo_engine.h, a row count below 1, an unknown PA kind and a zero or
    non-finite alpha with MIMO_EINVAL and a message -- on a machine without a GPU, so no
    allocation and no HIP call comes first (mimo_ofdm_rx used to read in front of its buffer
    for cp_len < 0; a negative n became a huge allocation)."""
    lib = _engine.lib()
    assert _seam_call(name, *args) == -1  # MIMO_EINVAL
    assert msg in lib.mimo_last_error().decode()


@pytest.mark.parametrize("name,args", [
    ("mimo_qam_map", (16, 0)), ("mimo_qam_slice", (4096, 0)), ("mimo_qam_llr", (64, 0)), ("mimo_fft", (64, 0)),
    ("mimo_ofdm_tx", (128, 64, 4, 0)), ("mimo_ofdm_rx", (128, 64, 0, 0)), ("mimo_ofdm_rx", (8192, 8190, 8192, 0)),
    ("mimo_pa", (2, 0)), ("mimo_mrt_precode", (4, 0)), ("mimo_combine", (4, 0)), ("mimo_awgn", (0,)),
])
def test_fine_seams_accept_a_size_of_zero_without_a_gpu(name, args):
    """A size of 0 is MIMO_OK with no HIP call (this machine has no GPU to answer one)."""
    assert _seam_call(name, *args) == 0


def test_count_bit_errors_of_nothing_is_zero_without_a_gpu():
    assert _seam_call("mimo_count_bit_errors", 0) == (0, 0)


def test_seam_wrappers_reject_mismatched_shapes():
    """_engine's wrappers size the library's reads from one argument: a second array of
    another shape, a last axis that is not n_fft + cp_len, or a matrix that is not 2-D is a
    ValueError before the library is called (no GPU needed to see it)."""
    z = np.zeros((4, 8), complex)
    with pytest.raises(ValueError, match="same shape"):
        _engine.combine(z, np.zeros((4, 9), complex))
    with pytest.raises(ValueError, match="same shape"):
        _engine.combine(z, np.zeros((3, 8), complex))
    with pytest.raises(ValueError, match="2-D"):
        _engine.combine(np.zeros(8, complex), np.zeros(8, complex))
    with pytest.raises(ValueError, match="2-D"):
        _engine.combine(np.zeros((2, 2, 2), complex), np.zeros((2, 2, 2), complex))
    with pytest.raises(ValueError, match="2-D"):
        _engine.mrt_precode(np.zeros(8, complex))
    with pytest.raises(ValueError, match="2-D"):
        _engine.mrt_precode(np.zeros((2, 2, 2), complex))
    with pytest.raises(ValueError, match="same number of elements"):
        _engine.count_bit_errors(np.zeros(8, int), np.zeros(9, int))
    with pytest.raises(ValueError, match="n_fft \\+ cp_len"):
        _engine.ofdm_rx(np.zeros((2, 131), complex), 128, 64, 4)
    with pytest.raises(ValueError, match="n_fft \\+ cp_len"):
        _engine.ofdm_rx(np.zeros(264, complex), 128, 64, 4)  # two symbols flattened
    with pytest.raises(ValueError, match="n_fft \\+ cp_len"):
        _engine.ofdm_rx(np.complex128(1.0), 128, 64, 4)
    with pytest.raises(ValueError, match="n_sub_carr"):
        _engine.ofdm_tx(np.zeros((2, 63), complex), 128, 64, 4)
