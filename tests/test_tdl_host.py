"""Host side of the channel bank and the TDL channel (mimo_engine_set_channel_bank,
mimo_engine_set_tdl, mimo_tdl_channels), no GPU: every argument the entry points refuse before any
HIP call, mimo_bank_capacity, the statistics of the CPU reference (tests/tdl_ref.py) on its own, and
the Python surface -- channel.MisoTdlFd, mp_model.Link, utilities.exp_pdp, sweep.py's options -- with
the CPU reference standing in for the fine seam."""
import copy
import ctypes

import numpy as np
import pytest

import _engine
import tdl_ref
from link_util import build_link

EINVAL = -1
_dp = ctypes.POINTER(ctypes.c_double)


def make_engine(channel, precision="f64", n_ant=4, n_sc=64, n_fft=128, reroll=True):
    tab = np.ones((n_ant, n_fft), complex) if channel == "table" else None
    return _engine.Engine(n_ant, n_sc, n_fft, 16, 4, channel, "cnc", np.zeros((n_ant, 3)), (10.0, 10.0, 1.5), 10.0,
                          np.full(n_fft, 3.5e9), reroll=reroll, precision=precision, chan_table=tab)


def point(eng, csi_eps=None):
    eng.set_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9, csi_eps=csi_eps)


def refused(word):
    return pytest.raises(_engine.EngineError, match=word)


# ---------------------------------------------------------------- capacity
@pytest.mark.parametrize("n_ant,n_sc,f64,f32", [(64, 1024, 1024, 2048), (3, 100, 223696, 447392), (4096, 8188, 2, 4)])
def test_bank_capacity(n_ant, n_sc, f64, f32):
    """floor(2^30 / (n_ant n_sub_carr 16 | 8)): config 2, a small generic shape, the largest system."""
    assert (1 << 30) // (n_ant * n_sc * 16) == f64 and (1 << 30) // (n_ant * n_sc * 8) == f32
    assert _engine.bank_capacity(n_ant, n_sc, "f64") == f64
    assert _engine.bank_capacity(n_ant, n_sc, "f32") == f32
    lib = _engine.lib()
    for bad, word in (((0, 4, 0), "n_ant"), ((4, 0, 0), "n_sub_carr"), ((4, 4, 2), "precision")):
        assert lib.mimo_bank_capacity(*bad) == EINVAL and word in lib.mimo_last_error().decode()


# ---------------------------------------------------------------- refusals: the bank
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_bank_refusals_name_their_field(prec):
    eng = make_engine("table", prec)
    lib, h = eng._L, eng._h
    good = np.ones((2, 4, 128), complex)
    eng.set_channel_bank(good)
    eng.set_channel_bank(None)  # n_bank = 0
    assert lib.mimo_engine_set_channel_bank(h, 2, None) == EINVAL and "tables" in lib.mimo_last_error().decode()
    assert lib.mimo_engine_set_channel_bank(h, -1, None) == EINVAL and "n_bank" in lib.mimo_last_error().decode()
    for bad in (np.nan, np.inf):
        t = good.copy()
        t[1, 2, 5] = bad * 1j
        with refused("tables must be finite .entry 1, antenna 2."):
            eng.set_channel_bank(t)
    with pytest.raises(ValueError, match="n_bank, n_ant, n_fft"):
        eng.set_channel_bank(np.ones((2, 4, 64), complex))
    for kind in ("rayleigh", "los", "tdl"):
        with refused("channel_kind"):
            make_engine(kind, prec).set_channel_bank(good)


@pytest.mark.parametrize("prec,cap", [("f64", 2), ("f32", 4)])
def test_bank_above_capacity_is_refused_before_the_tables_are_read(prec, cap):
    eng = make_engine("table", prec, n_ant=4096, n_sc=8188, n_fft=8192)
    assert _engine.bank_capacity(4096, 8188, prec) == cap
    dummy = np.zeros(2)
    rc = eng._L.mimo_engine_set_channel_bank(eng._h, cap + 1, dummy.ctypes.data_as(_dp))
    msg = eng._L.mimo_last_error().decode()
    assert rc == EINVAL and "n_bank" in msg and f"[0, {cap}]" in msg


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_csi_error_on_a_bank_is_refused_before_any_hip_call(prec):
    """... for n_bank > 1 only: one table, as a bank of one or as the create-time table, keeps the
    table engine's shared estimate (those runs need a GPU and are not made here)."""
    eng = make_engine("table", prec)
    eng.set_channel_bank(np.ones((2, 4, 128), complex))
    point(eng, csi_eps=0.1)
    with refused("csi_eps"):
        eng.run(1, 0, 4, [0])
    pt = eng.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9, csi_eps=0.1)
    with refused("csi_eps"):
        eng.run_points([pt, pt], [1, 2], [0, 0], [2, 2], [0])
    if prec == "f64":
        with refused("csi_eps"):
            eng.measure_points([pt], [1], [0], [2], [0])


# ---------------------------------------------------------------- refusals: the TDL profile
def test_tdl_engine_refusals_name_their_field():
    with pytest.raises(ValueError, match="reroll_chan"):
        make_engine("tdl", reroll=False)
    eng = make_engine("tdl")
    point(eng)
    with refused("mimo_engine_set_tdl"):  # no profile yet
        eng.run(1, 0, 4, [0])
    eng.set_tdl([0, 3], [0.5, 0.5])
    point(eng, csi_eps=0.2)
    with refused("csi_eps"):
        eng.run(1, 0, 4, [0])
    for kind in ("rayleigh", "table"):
        with refused("channel_kind"):
            make_engine(kind).set_tdl([0], [1.0])
    assert eng._L.mimo_engine_set_tdl(eng._h, None) == EINVAL and "profile" in eng._L.mimo_last_error().decode()


BAD_PROFILES = [("no_taps", [], [], None, "n_taps"), ("taps65", list(range(65)), [1.0] * 65, None, "n_taps"),
                ("negative", [-1, 2], [1, 1], None, "delays"), ("at_n_fft", [0, 128], [1, 1], None, "delays"),
                ("equal", [0, 3, 3], [1, 1, 1], None, "delays"), ("descending", [4, 2], [1, 1], None, "delays"),
                ("power0", [0, 1], [1, 0.0], None, "powers"), ("power_neg", [0, 1], [1, -1.0], None, "powers"),
                ("power_nan", [0, 1], [np.nan, 1], None, "powers"), ("power_inf", [0, 1], [1, np.inf], None, "powers"),
                ("amp0", [0], [1.0], [1, 1, 0.0, 1], "ant_amp"), ("amp_nan", [0], [1.0], [1, np.nan, 1, 1], "ant_amp")]


@pytest.mark.parametrize("name,delays,powers,amp,word", BAD_PROFILES, ids=[b[0] for b in BAD_PROFILES])
def test_every_profile_rule_is_refused_by_name(name, delays, powers, amp, word):
    """... by mimo_engine_set_tdl and by the seam alike, before any HIP call."""
    eng = make_engine("tdl")
    with refused(word):
        eng.set_tdl(delays, powers, amp)
    with refused(word):
        _engine.tdl_channels(delays, powers, 4, 128, 1, 0, 2, ant_amp=amp)


def test_seam_refusals_and_null_pointers():
    lib = _engine.lib()
    prof = _engine.TdlProfile([0, 2], [0.5, 0.5])
    h = np.zeros(2 * 4 * 128 * 2)
    ref = ctypes.byref(prof)
    for (a, f, n), word in (((0, 128, 1), "n_ant"), ((4, 96, 1), "n_fft"), ((4, 16384, 1), "n_fft"), ((4, 128, -1), "n ")):
        assert lib.mimo_tdl_channels(ref, a, f, 1, 0, n, h.ctypes.data_as(_dp), None) == EINVAL
        assert word in lib.mimo_last_error().decode(), lib.mimo_last_error().decode()
    assert lib.mimo_tdl_channels(ref, 4, 128, 1, 0, 1, None, None) == EINVAL and "h_out" in lib.mimo_last_error().decode()
    assert lib.mimo_tdl_channels(None, 4, 128, 1, 0, 1, h.ctypes.data_as(_dp), None) == EINVAL
    assert "profile" in lib.mimo_last_error().decode()
    for field in ("delays", "powers"):
        p = _engine.TdlProfile([0, 2], [0.5, 0.5])
        setattr(p, field, None)
        assert lib.mimo_tdl_channels(ctypes.byref(p), 4, 128, 1, 0, 1, h.ctypes.data_as(_dp), None) == EINVAL
        assert field in lib.mimo_last_error().decode()
    assert _engine.tdl_channels([0, 2], [0.5, 0.5], 4, 128, 1, 0, 0).shape == (0, 4, 128)  # n = 0: nothing to do
    assert lib.mimo_engine_last_chan_ms(make_engine("tdl")._h) == 0.0


# ---------------------------------------------------------------- the reference's own statistics
N_REAL, N_ANT, N_FFT = 512, 4, 128
POWERS = np.array([0.75, 0.75])  # two equal taps at delays 0 and 8, P = 1.5 (not normalised on purpose)


@pytest.fixture(scope="module")
def ref_h():
    return tdl_ref.tdl_channels([0, 8], POWERS, N_ANT, N_FFT, 0xC0FFEE, 0, N_REAL)


def test_reference_mean_power(ref_h):
    """Mean |H|^2 = P = sum powers, one sample per (realisation, antenna) since the sub-carriers of
    one are correlated: |H|^2 is exponential with variance P^2, so 5 standard errors."""
    P = float(POWERS.sum())
    tol = 5 * P / np.sqrt(N_REAL * N_ANT)
    for n in (0, 5, 127):
        m = float(np.mean(np.abs(ref_h[:, :, n]) ** 2))
        print(f"bin {n}: mean |H|^2 {m:.4f}, P {P}, tolerance {tol:.4f}")
        assert abs(m - P) <= tol


def test_reference_lag4_correlation(ref_h):
    """E H[n + 4] conj(H[n]) = sum_l powers[l] exp(-2j pi 4 d_l / F) = P (1 - j) / 2 for delays 0 and
    8 at F 128.  A generator that ignored the delays would give P, an i.i.d. one 0: both are
    several tolerances away."""
    P = float(POWERS.sum())
    tol = 5 * np.sqrt(2) * P / np.sqrt(N_REAL * N_ANT)
    want = P * (1 - 1j) / 2
    assert abs(want - P) > 3 * tol and abs(want) > 3 * tol
    for n in (0, 60, 123):
        c = complex(np.mean(ref_h[:, :, n + 4] * np.conj(ref_h[:, :, n])))
        print(f"bin {n}: lag-4 correlation {c:.4f}, expected {want:.4f}, tolerance {tol:.4f}")
        assert abs(c - want) <= tol


def test_reference_single_tap_and_float64_yardstick():
    """One tap at delay 0 is flat at the tap; at delay d it turns by exp(-2j pi n d / F); the
    float64 taps agree with the long-double ones to rounding."""
    h, g = tdl_ref.tdl_channels([0], [2.0], 3, 128, 5, 7, 2, ant_amp=[1.0, 0.5, 2.0], taps=True)
    np.testing.assert_array_equal(h, np.broadcast_to(g, h.shape))
    h5, g5 = tdl_ref.tdl_channels([5], [2.0], 3, 128, 5, 7, 2, ant_amp=[1.0, 0.5, 2.0], taps=True)
    np.testing.assert_array_equal(g5, g)
    # (float64 yardstick: the angle reduced first, its rounding then stays below 2^-52 |g| 2 pi)
    np.testing.assert_allclose(h5, g * np.exp(-2j * np.pi * ((5 * np.arange(128)) % 128) / 128), rtol=0,
                               atol=8 * 2.0 ** -52 * np.abs(g).max())
    np.testing.assert_allclose(tdl_ref.np_taps([2.0], 3, 5, [7, 8], [1.0, 0.5, 2.0]), g, rtol=1e-14)
    # trial indices wrap at 2^32
    np.testing.assert_array_equal(tdl_ref.tdl_channels([0], [2.0], 3, 128, 5, 2 ** 32 + 7, 1), tdl_ref.tdl_channels(
        [0], [2.0], 3, 128, 5, 7, 1))


# ---------------------------------------------------------------- Python surface
@pytest.fixture
def cpu_seam(monkeypatch):
    """The CPU reference in the fine seam's place, recording its calls."""
    calls = []

    def fake(*a, **k):
        calls.append((a, k))
        return tdl_ref.tdl_channels(*a, **k)

    monkeypatch.setattr(_engine, "tdl_channels", fake)
    return calls


def tdl_link(delays=(0, 2, 5), powers_db=(0.0, -3.0, -6.0), **kw):
    import channel
    import mp_model
    base, mod = build_link(**kw)
    ch = channel.MisoTdlFd(base.my_array.array_elements, base.my_standard_rx, delays, powers_db, seed=77)
    link = mp_model.Link(mod_obj=mod, array_obj=base.my_array, std_rx_obj=base.my_standard_rx, chan_obj=ch,
                         noise_obj=copy.deepcopy(base.my_noise), rx_loc_var=10.0, n_err_min=10, bits_sent_max=1000,
                         device=kw.get("device"))
    link.update_distortion(ibo_val_db=1.0)
    return link, ch


def test_exp_pdp():
    from utilities import exp_pdp
    d, p = exp_pdp(8, 4, 3.0)
    assert d.tolist() == [0, 4, 8, 12, 16, 20, 24, 28] and d.dtype == np.int32
    assert p.sum() == pytest.approx(1.0, abs=1e-15)
    np.testing.assert_allclose(10 * np.log10(p[1:] / p[:-1]), -3.0, atol=1e-12)
    d1, p1 = exp_pdp(1, 1, 0.0)
    assert d1.tolist() == [0] and p1.tolist() == [1.0]
    for bad in ((0, 1, 1.0), (2, 0, 1.0), (2, 1, -1.0), (2, 1, np.nan)):
        with pytest.raises(ValueError):
            exp_pdp(*bad)


def test_miso_tdl_fd_surface_and_validation(cpu_seam):
    import channel
    base, _ = build_link(n_ant=4)
    tx, rx = base.my_array.array_elements, base.my_standard_rx
    ch = channel.MisoTdlFd(tx, rx, [0, 2, 5], [0.0, -3.0, -6.0], seed=77)
    assert str(ch) == "tdl" and ch.n_inputs == 4 and ch.fd_samp_size == 128
    np.testing.assert_allclose(ch.powers, [1.0, 10 ** -0.3, 10 ** -0.6])
    # ant_amp: MisoRayleighFd's attenuation at the centre frequency (bin 0 of the carrier grid)
    ray = channel.MisoRayleighFd(tx, rx, seed=1)
    np.testing.assert_allclose(ch.ant_amp, ray.los_fd_att_mat[:, 0], rtol=1e-14)
    h0 = ch.get_channel_mat_fd()
    assert h0.shape == (4, 128) and ch.n_drawn == 1
    np.testing.assert_array_equal(h0, tdl_ref.tdl_channels(ch.delays, ch.powers, 4, 128, 77, 0, 1, ant_amp=ch.ant_amp)[0])
    ch.reroll_channel_coeffs()
    assert cpu_seam[-1][0][4:7] == (77, 1, 1) and not np.array_equal(ch.channel_mat_fd, h0)
    ch.reroll_channel_coeffs(skip_attenuation=True)
    assert cpu_seam[-1][1]["ant_amp"] is None
    ch.set_channel_mat_fd(h0)
    assert ch.get_channel_mat_fd() is h0
    out = ch.propagate(np.ones((4, 128)), sum_signals=False)
    np.testing.assert_array_equal(out, h0)
    for delays, pdb in (([], []), (list(range(65)), [0.0] * 65), ([0, 0], [0, 0]), ([3, 1], [0, 0]), ([0, 128], [0, 0]),
                        ([-1, 4], [0, 0]), ([0.5, 2], [0, 0]), ([0, 1], [0.0]), ([0, 1], [0.0, np.nan])):
        with pytest.raises(ValueError):
            channel.MisoTdlFd(tx, rx, delays, pdb)


def test_link_picks_the_tdl_engine(cpu_seam, monkeypatch):
    """reroll_chan=True: a TDL engine with the object's profile (amplitudes relative to the
    strongest antenna); reroll_chan=False: the table engine on the object's current matrix."""
    seen = []

    class Capture:
        def __init__(self, *a, **k):
            seen.append(dict(args=a, kw=k, tdl=None))

        def set_point(self, *a, **k):
            pass

        def set_tdl(self, *a):
            seen[-1]["tdl"] = a

    monkeypatch.setattr(_engine, "Engine", Capture)
    link, ch = tdl_link(n_ant=4, device=0)
    link.engine(reroll_chan=True)
    assert seen[-1]["args"][5] == "tdl" and seen[-1]["kw"]["chan_table"] is None and seen[-1]["kw"]["reroll"] is True
    delays, powers, amp = seen[-1]["tdl"]
    np.testing.assert_array_equal(delays, [0, 2, 5])
    np.testing.assert_array_equal(powers, link.my_miso_chan.powers)
    np.testing.assert_allclose(amp, ch.ant_amp / ch.ant_amp.max(), rtol=1e-15)
    assert amp.max() == 1.0
    n = len(seen)
    link.engine(reroll_chan=True)
    assert len(seen) == n  # the same engine serves the next call
    link.engine(reroll_chan=False)
    assert seen[-1]["args"][5] == "table" and seen[-1]["tdl"] is None
    np.testing.assert_array_equal(seen[-1]["kw"]["chan_table"], link.my_miso_chan.channel_mat_fd)


def test_sweep_parses_the_tdl_channel(cpu_seam):
    import sweep
    ap = sweep.build_parser()
    for grid in ap._option_string_actions["--grid"].choices:
        args = ap.parse_args(["--grid", grid, "--channel", "tdl", "--tdl-taps", "5", "--tdl-step", "3",
                              "--tdl-decay-db", "1.5"])
        assert (args.channel, args.tdl_taps, args.tdl_step, args.tdl_decay_db) == ("tdl", 5, 3, 1.5)
    d = ap.parse_args(["--channel", "tdl"])
    assert (d.tdl_taps, d.tdl_step, d.tdl_decay_db) == (8, 4, 3.0)
    assert ap.parse_args([]).channel == "rayleigh"
    base, _ = build_link(n_ant=4)
    ch = sweep.make_channel("tdl", base.my_array.array_elements, base.my_standard_rx, (5, 3, 1.5))
    assert str(ch) == "tdl" and ch.delays.tolist() == [0, 3, 6, 9, 12] and ch.powers.sum() == pytest.approx(1.0)
    assert str(sweep.make_channel("rayleigh", base.my_array.array_elements, base.my_standard_rx)) == "rayleigh"
    assert sweep.RESIDUAL_DISTORTION["tdl"] is None
