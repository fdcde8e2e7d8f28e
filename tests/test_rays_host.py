"""Host side of the ray-cluster channel (mimo_engine_set_rays, mimo_rays_channels), no GPU: every
argument the entry points refuse before any HIP call, the statistics of the CPU reference
(tests/rays_ref.py) on its own, utilities.ring_clusters and scatterer_steering, and the Python
surface -- channel.MisoRaysFd, mp_model.Link, sweep.py's options -- with the CPU reference standing in
for the fine seam."""
import copy
import ctypes

import numpy as np
import pytest

import _engine
import rays_ref
from link_util import build_link

EINVAL = -1
_dp = ctypes.POINTER(ctypes.c_double)
N_ANT, N_FFT = 4, 128


def make_engine(channel="tdl", precision="f64", n_ant=N_ANT, n_sc=64, n_fft=N_FFT):
    tab = np.ones((n_ant, n_fft), complex) if channel == "table" else None
    return _engine.Engine(n_ant, n_sc, n_fft, 16, 4, channel, "cnc", np.zeros((n_ant, 3)), (10.0, 10.0, 1.5), 10.0,
                          np.full(n_fft, 3.5e9), reroll=True, precision=precision, chan_table=tab)


def point(eng, csi_eps=None):
    eng.set_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9, csi_eps=csi_eps)


def good(n_ant=N_ANT):
    """delays, ray_tap, ray_amp, steer, ray_kind of a valid profile: 2 taps, rays 3 + 1."""
    steer = np.exp(1j * np.arange(n_ant * 4).reshape(n_ant, 4))
    return dict(delays=[0, 3], ray_tap=[0, 0, 0, 1], ray_amp=[0.5, 0.25, 1.0, 0.7], steer=steer, ray_kind=[0, 1, 0, 0])


def raw(prof, eng=None):
    """(rc, message) of the raw C call: the setter on ``eng``, or the seam with n = 1."""
    lib = _engine.lib()
    ref = ctypes.byref(prof) if prof is not None else None
    if eng is not None:
        rc = lib.mimo_engine_set_rays(eng._h, ref)
    else:
        h = np.zeros(N_ANT * N_FFT * 2)
        rc = lib.mimo_rays_channels(ref, N_ANT, N_FFT, 1, 0, 1, h.ctypes.data_as(_dp), None, None)
    return rc, lib.mimo_last_error().decode()


# ---------------------------------------------------------------- refusals
def test_symbols_and_limits():
    assert {"mimo_engine_set_rays", "mimo_rays_channels"} <= set(_engine.SYMBOLS)
    assert _engine.RAYS_MAX == 1024
    assert ctypes.sizeof(_engine.RayProfile) == 56  # mimo_rays on LP64: 4 (+4) 8 4 (+4) 8 8 8 8


def test_engine_kind_and_null_profile():
    eng = make_engine()
    eng.set_rays(**good())
    for kind in ("rayleigh", "table"):
        with pytest.raises(_engine.EngineError, match="channel_kind"):
            make_engine(kind).set_rays(**good())
    for e in (eng, None):
        rc, msg = raw(None, e)
        assert rc == EINVAL and "profile" in msg
    assert _engine.lib().mimo_engine_set_rays(None, None) == EINVAL


@pytest.mark.parametrize("field", ["delays", "ray_tap", "ray_amp", "steer"])
def test_null_required_arrays(field):
    eng = make_engine()
    for e in (eng, None):
        prof = _engine.RayProfile(**good())
        setattr(prof, field, None)
        rc, msg = raw(prof, e)
        assert rc == EINVAL and field in msg, msg
    prof = _engine.RayProfile(**good())
    prof.ray_kind = None  # optional: all diffuse
    assert raw(prof, eng)[0] == 0


def _with(**kw):
    g = good()
    g.update(kw)
    return g


def _steer_bad(a, r, v):
    s = good()["steer"].copy()
    s[a, r] = v
    return s


BAD = [
    ("taps0", dict(n_taps=0), "n_taps"), ("taps65", dict(n_taps=65), "n_taps"),
    ("rays_below_taps", dict(n_rays=1), "n_rays"), ("rays1025", dict(n_rays=1025), "n_rays"),
    ("delay_neg", _with(delays=[-1, 3]), "delays"), ("delay_at_n_fft", _with(delays=[0, N_FFT]), "delays"),
    ("delay_equal", _with(delays=[3, 3]), "delays"), ("delay_desc", _with(delays=[4, 2]), "delays"),
    ("tap_start", _with(ray_tap=[1, 1, 1, 1]), "ray_tap"), ("tap_desc", _with(ray_tap=[0, 1, 0, 1]), "ray_tap"),
    ("tap_jump", _with(delays=[0, 3, 5], ray_tap=[0, 0, 2, 2]), "ray_tap"),
    ("tap_short", _with(ray_tap=[0, 0, 0, 0]), "ray_tap"), ("tap_past", _with(ray_tap=[0, 1, 1, 2]), "ray_tap"),
    ("amp0", _with(ray_amp=[0.5, 0.0, 1, 1]), "ray_amp"), ("amp_neg", _with(ray_amp=[0.5, -1.0, 1, 1]), "ray_amp"),
    ("amp_nan", _with(ray_amp=[np.nan, 1, 1, 1]), "ray_amp"), ("amp_inf", _with(ray_amp=[1, 1, 1, np.inf]), "ray_amp"),
    ("kind2", _with(ray_kind=[0, 2, 0, 0]), "ray_kind"), ("kind255", _with(ray_kind=[0, 0, 0, 255]), "ray_kind"),
    ("steer_nan", _with(steer=_steer_bad(2, 1, np.nan)), r"steer.*antenna 2, ray 1"),
    ("steer_inf_im", _with(steer=_steer_bad(3, 0, 1j * np.inf)), r"steer.*antenna 3, ray 0"),
]


@pytest.mark.parametrize("name,spec,word", BAD, ids=[b[0] for b in BAD])
def test_every_profile_rule_is_refused_by_name(name, spec, word):
    """... by mimo_engine_set_rays and by the seam alike, through the raw C calls, before any HIP call."""
    import re
    eng = make_engine()
    for e in (eng, None):
        if "delays" in spec:
            prof = _engine.RayProfile(**spec)
        else:  # a count out of range: a good profile's arrays (sized for the larger count where read)
            g = good()
            n = max(spec.get("n_rays", 4), 4)
            g.update(ray_tap=[0] * (n - 1) + [1], ray_amp=[1.0] * n, steer=np.ones((N_ANT, n)), ray_kind=[0] * n)
            prof = _engine.RayProfile(**g)
            for k, v in spec.items():
                setattr(prof, k, v)
        rc, msg = raw(prof, e)
        assert rc == EINVAL and re.search(word, msg), msg


def test_seam_sizes_and_null_pointers():
    lib = _engine.lib()
    prof = _engine.RayProfile(**good())
    h = np.zeros(2 * N_ANT * N_FFT * 2)
    ref = ctypes.byref(prof)
    for (a, f, n), word in (((0, 128, 1), "n_ant"), ((4, 96, 1), "n_fft"), ((4, 16384, 1), "n_fft"), ((4, 128, -1), "n ")):
        assert lib.mimo_rays_channels(ref, a, f, 1, 0, n, h.ctypes.data_as(_dp), None, None) == EINVAL
        assert word in lib.mimo_last_error().decode(), lib.mimo_last_error().decode()
    assert lib.mimo_rays_channels(ref, 4, 128, 1, 0, 1, None, None, None) == EINVAL
    assert "h_out" in lib.mimo_last_error().decode()
    g = good()
    out = _engine.rays_channels(g["delays"], g["ray_tap"], g["ray_amp"], g["steer"], 128, 1, 0, 0, taps=True, gains=True)
    assert [o.shape for o in out] == [(0, 4, 128), (0, 4, 2), (0, 4)]  # n = 0: nothing to do


def test_runs_are_refused_before_any_hip_call():
    eng = make_engine()
    point(eng)
    with pytest.raises(_engine.EngineError, match="mimo_engine_set_rays"):  # no profile yet
        eng.run(1, 0, 4, [0])
    eng.set_rays(**good())
    point(eng, csi_eps=0.2)
    with pytest.raises(_engine.EngineError, match="csi_eps"):
        eng.run(1, 0, 4, [0])
    assert eng.chan_kernel_ms == 0.0


def test_python_argument_errors():
    eng = make_engine()
    g = good()
    for bad in (dict(steer=np.ones((3, 4))), dict(steer=np.ones((4, 5))), dict(steer=np.ones(4)),
                dict(ray_amp=[1.0, 1.0]), dict(ray_kind=[0, 1]), dict(ray_kind=[0, 0.5, 0, 0]),
                dict(ray_tap=[0, 0.5, 1, 1]), dict(delays=[[0, 3]]), dict(delays=[0, 2 ** 31])):
        with pytest.raises(ValueError):
            eng.set_rays(**{**g, **bad})


# ---------------------------------------------------------------- the reference's own statistics
N_TRIALS = 20000


@pytest.fixture(scope="module")
def stat_profile():
    """A = 4; tap 0: 3 diffuse rays and 1 specular, tap 1: 1 diffuse ray; complex non-unit steering."""
    rng = np.random.default_rng(5)
    steer = (0.5 + rng.random((N_ANT, 5))) * np.exp(2j * np.pi * rng.random((N_ANT, 5)))
    ray_tap = np.array([0, 0, 0, 0, 1])
    amp = np.array([0.6, 0.4, 0.8, 0.9, 0.7])
    kind = np.array([0, 0, 1, 0, 0])
    gains = rays_ref.ld_gains(amp, 0xC0FFEE, np.arange(N_TRIALS), kind)
    taps = rays_ref.ld_taps_of(gains, ray_tap, steer).astype(np.complex128)  # [N, A, 2]
    return steer, ray_tap, amp, kind, taps


def test_reference_tap_correlation(stat_profile):
    """Sample E g_l g_l^H against R_l = S_l diag(amp^2) S_l^H, entry by entry within five standard
    errors.  With independent, zero-mean, circular gains of power p_r = amp_r^2 and fourth moment
    m_r (2 p_r^2 diffuse, p_r^2 specular) the product X = g[a] conj(g[b]) has
    E |X - R_ab|^2 = R_aa R_bb + sum_r (m_r - 2 p_r^2) |s_ar|^2 |s_br|^2: R_aa R_bb less the
    specular rays' p_r^2 |s_ar s_br|^2."""
    steer, ray_tap, amp, kind, taps = stat_profile
    for l in (0, 1):
        sel = ray_tap == l
        S, p = steer[:, sel], amp[sel] ** 2
        R = (S * p) @ S.conj().T
        spec = kind[sel] == 1
        less = np.einsum("r,ar,br->ab", p[spec] ** 2, np.abs(S[:, spec]) ** 2, np.abs(S[:, spec]) ** 2)
        var = np.outer(R.diagonal().real, R.diagonal().real) - less
        assert np.all(var > 0)
        tol = 5 * np.sqrt(var / N_TRIALS)
        got = np.einsum("na,nb->ab", taps[:, :, l], taps[:, :, l].conj()) / N_TRIALS
        worst = float(np.max(np.abs(got - R) / tol))
        print(f"tap {l}: worst |sample - R| / tolerance {worst:.3f}; |R| {np.abs(R).min():.3f} ... {np.abs(R).max():.3f}")
        assert worst <= 1.0
        # taps independent from antenna to antenna would give a diagonal R: tap 1's, of one ray, has
        # rank one, |R_ab| = p |s_a| |s_b|, and every off-diagonal entry is many tolerances from 0
        if l == 1:
            assert np.all((np.abs(R) > 10 * tol)[~np.eye(N_ANT, dtype=bool)])


def test_reference_taps_are_uncorrelated(stat_profile):
    """E g_0[a] conj(g_1[b]) = 0 with variance R0_aa R1_bb (disjoint, independent rays)."""
    steer, ray_tap, amp, kind, taps = stat_profile
    p = amp ** 2
    r0 = np.sum(np.abs(steer[:, ray_tap == 0]) ** 2 * p[ray_tap == 0], axis=1)
    r1 = np.sum(np.abs(steer[:, ray_tap == 1]) ** 2 * p[ray_tap == 1], axis=1)
    tol = 5 * np.sqrt(np.outer(r0, r1) / N_TRIALS)
    got = np.einsum("na,nb->ab", taps[:, :, 0], taps[:, :, 1].conj()) / N_TRIALS
    print(f"cross-tap: worst / tolerance {float(np.max(np.abs(got) / tol)):.3f}")
    assert np.all(np.abs(got) <= tol)


def test_reference_single_specular_ray_and_float64_yardstick():
    steer = np.array([[1.5 * np.exp(0.3j)], [0.25 * np.exp(-2j)], [1.0]])
    h, g, c = rays_ref.rays_channels([0], [0], [0.8], steer, 128, 9, 2 ** 32 - 2, 5, ray_kind=[1], taps=True, gains=True)
    np.testing.assert_allclose(np.abs(c), 0.8, rtol=4 * 2.0 ** -52)
    np.testing.assert_allclose(np.abs(g[:, :, 0]), np.broadcast_to(0.8 * np.abs(steer[:, 0]), (5, 3)),
                               rtol=8 * 2.0 ** -52)
    np.testing.assert_array_equal(h, np.broadcast_to(g, h.shape))  # one tap at delay 0: flat
    assert len({complex(v) for v in c[:, 0]}) == 5
    # trial indices wrap at 2^32
    np.testing.assert_array_equal(rays_ref.rays_channels([0], [0], [0.8], steer, 128, 9, 0, 3, ray_kind=[1]), h[2:])
    amp, kind = np.array([0.5, 2.0, 1.0]), np.array([0, 1, 0])
    np.testing.assert_allclose(rays_ref.np_gains(amp, 5, [7, 8], kind), rays_ref.ld_gains(amp, 5, [7, 8], kind).astype(complex),
                               rtol=1e-14)
    # a diffuse ray is the TDL tap's formula on stream 8, antenna word 0
    from oracle import philox as px
    w0, w1 = rays_ref.ray_words(5, [7], 3)
    np.testing.assert_array_equal(rays_ref.np_gains(np.ones(3), 5, [7]), px.box_muller(w0, w1))


# ---------------------------------------------------------------- utilities
def test_ring_clusters_offsets_and_powers():
    from utilities import ring_clusters
    delays, powers, az = [0, 4, 9], np.array([0.5, 0.3, 0.2]), [30.0, 90.0, 140.0]
    for m in (2, 3, 20):
        tap, amp, kind, pts = ring_clusters(delays, powers, az, 5.0, m, 300.0, z=1.5)
        assert tap.dtype == np.int32 and tap.tolist() == sorted(tap.tolist()) and np.all(np.bincount(tap) == m)
        assert pts.shape == (3 * m, 3) and np.all(kind == 0) and np.all(pts[:, 2] == 1.5)
        np.testing.assert_allclose(np.hypot(pts[:, 0], pts[:, 1]), 300.0, rtol=1e-14)
        ang = np.rad2deg(np.arctan2(pts[:, 1], pts[:, 0])).reshape(3, m)
        off = ang - np.asarray(az)[:, None]
        np.testing.assert_allclose(off.mean(1), 0.0, atol=1e-10)
        np.testing.assert_allclose(np.sqrt(np.mean(off ** 2, axis=1)), 5.0, rtol=1e-10)      # rms: the spread
        np.testing.assert_allclose(np.diff(off, axis=1), np.diff(off, axis=1)[0, 0], rtol=1e-9)  # equally spaced
        assert np.abs(off).max() <= np.sqrt(3) * 5.0 * (1 + 1e-12)
        np.testing.assert_allclose(np.bincount(tap, weights=amp ** 2), powers, rtol=1e-14)
    # M = 1: one ray per cluster at the cluster's azimuth
    tap, amp, kind, pts = ring_clusters(delays, powers, az, 5.0, 1, 300.0)
    assert tap.tolist() == [0, 1, 2]
    np.testing.assert_allclose(np.rad2deg(np.arctan2(pts[:, 1], pts[:, 0])), az, rtol=1e-13)
    np.testing.assert_allclose(amp ** 2, powers, rtol=1e-14)
    # a K factor: the specular ray first, in tap 0, and the total power unchanged
    tap, amp, kind, pts = ring_clusters(delays, powers, az, 5.0, 4, 300.0, k_db=6.0, los_point=(212.0, 212.0, 1.5))
    k = 10 ** 0.6
    assert tap[:2].tolist() == [0, 0] and kind.tolist() == [1] + [0] * 12 and pts[0].tolist() == [212.0, 212.0, 1.5]
    assert amp[0] ** 2 == pytest.approx(k / (k + 1) * powers.sum(), rel=1e-14)
    np.testing.assert_allclose(np.bincount(tap[1:], weights=amp[1:] ** 2), powers / (k + 1), rtol=1e-14)
    assert np.sum(amp ** 2) == pytest.approx(powers.sum(), rel=1e-14)
    for bad in (dict(rays_per_cluster=0), dict(spread_deg=-1.0), dict(radius=0.0), dict(k_db=3.0), dict(az_deg=[1.0]),
                dict(los_point=(1, 2, 3))):
        kw = dict(delays=delays, powers=powers, az_deg=az, spread_deg=5.0, rays_per_cluster=2, radius=300.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ring_clusters(**kw)


def test_scatterer_steering_is_the_los_phase():
    """At the receiver's position and the centre frequency: MisoLosFd(skip_attenuation=True)'s column 0."""
    import channel
    from utilities import scatterer_steering
    base, _ = build_link(n_ant=4)
    tx, rx = base.my_array.array_elements, base.my_standard_rx
    los = channel.MisoLosFd()
    los.calc_channel_mat(tx, rx, skip_attenuation=True)
    pos = np.asarray([[t.cord_x, t.cord_y, t.cord_z] for t in tx])
    f0 = channel.carrier_freqs(rx.modem.n_fft, rx.carrier_spacing, rx.center_freq)[0]
    s = scatterer_steering(pos, [[rx.cord_x, rx.cord_y, rx.cord_z], [0.0, 100.0, 1.5]], f0)
    assert s.shape == (4, 2)
    np.testing.assert_array_equal(s[:, 0], los.channel_mat_fd[:, 0])
    np.testing.assert_allclose(np.abs(s), 1.0, rtol=1e-15)


# ---------------------------------------------------------------- Python surface
@pytest.fixture
def cpu_seam(monkeypatch):
    """The CPU reference in the fine seam's place, recording its calls."""
    calls = []

    def fake(*a, **k):
        calls.append((a, k))
        return rays_ref.rays_channels(*a, **k)

    monkeypatch.setattr(_engine, "rays_channels", fake)
    return calls


def ring(n_taps=3, m=2, k_db=None):
    from utilities import exp_pdp, ring_clusters
    delays, powers = exp_pdp(n_taps, 2, 3.0)
    los = None if k_db is None else (212.0, 212.0, 1.5)
    return (delays,) + ring_clusters(delays, powers, np.linspace(30, 150, n_taps), 5.0, m, 300.0, z=1.5, k_db=k_db,
                                     los_point=los)


def test_miso_rays_fd_surface_and_validation(cpu_seam):
    import channel
    from utilities import scatterer_steering
    base, _ = build_link(n_ant=4)
    tx, rx = base.my_array.array_elements, base.my_standard_rx
    delays, tap, amp, kind, pts = ring(k_db=3.0)
    ch = channel.MisoRaysFd(tx, rx, delays, tap, amp, pts, ray_kind=kind, seed=77)
    assert str(ch) == "rays" and ch.n_inputs == 4 and ch.fd_samp_size == 128 and ch.n_drawn == 1
    ray = channel.MisoRayleighFd(tx, rx, seed=1)
    np.testing.assert_allclose(ch.ant_amp, ray.los_fd_att_mat[:, 0], rtol=1e-14)  # MisoTdlFd's ant_amp
    pos = np.asarray([[t.cord_x, t.cord_y, t.cord_z] for t in tx])
    f0 = channel.carrier_freqs(128, rx.carrier_spacing, rx.center_freq)[0]
    np.testing.assert_array_equal(ch.steer(True), scatterer_steering(pos, pts, f0))
    np.testing.assert_array_equal(ch.steer(), ch.steer(True) * ch.ant_amp[:, None])
    h0 = ch.get_channel_mat_fd()
    assert h0.shape == (4, 128)
    np.testing.assert_array_equal(h0, rays_ref.rays_channels(delays, tap, amp, ch.steer(), 128, 77, 0, 1, ray_kind=kind)[0])
    ch.reroll_channel_coeffs()
    assert cpu_seam[-1][0][5:8] == (77, 1, 1) and not np.array_equal(ch.channel_mat_fd, h0)
    ch.reroll_channel_coeffs(skip_attenuation=True)
    np.testing.assert_array_equal(cpu_seam[-1][0][3], ch.steer(True))
    ch.set_channel_mat_fd(h0)
    assert ch.get_channel_mat_fd() is h0
    np.testing.assert_array_equal(ch.propagate(np.ones((4, 128)), sum_signals=False), h0)
    assert np.all(channel.MisoRaysFd(tx, rx, delays, tap, amp, pts).ray_kind == 0)  # None: all diffuse
    ok = dict(delays=delays, ray_tap=tap, ray_amp=amp, points=pts, ray_kind=kind)
    for bad in (dict(delays=[]), dict(delays=[0, 0, 1]), dict(delays=[0, 1, 128]), dict(delays=[0.5, 1, 2]),
                dict(ray_tap=tap[::-1]), dict(ray_tap=np.minimum(tap, 1)), dict(ray_tap=tap[:-1]),
                dict(ray_amp=np.r_[amp[:-1], 0.0]), dict(ray_amp=np.r_[amp[:-1], np.nan]), dict(ray_amp=amp[:-1]),
                dict(points=pts[:, :2]), dict(points=np.r_[pts[:-1], [[np.inf, 0, 0]]]), dict(ray_kind=kind + 1),
                dict(ray_kind=kind[:-1]),
                dict(delays=np.arange(65), ray_tap=np.arange(65), ray_amp=np.ones(65), points=np.ones((65, 3)), ray_kind=None),
                dict(ray_tap=np.zeros(1025), delays=[0], ray_amp=np.ones(1025), points=np.ones((1025, 3)), ray_kind=None)):
        with pytest.raises(ValueError):
            channel.MisoRaysFd(tx, rx, **{**ok, **bad})


def test_link_runs_rays_on_the_tdl_engine(cpu_seam, monkeypatch):
    import channel
    import mp_model
    seen = []

    class Capture:
        def __init__(self, *a, **k):
            seen.append(dict(args=a, kw=k, rays=None, tdl=None))

        def set_point(self, *a, **k):
            pass

        def set_tdl(self, *a):
            seen[-1]["tdl"] = a

        def set_rays(self, *a):
            seen[-1]["rays"] = a

    monkeypatch.setattr(_engine, "Engine", Capture)
    base, mod = build_link(n_ant=4, device=0)
    delays, tap, amp, kind, pts = ring(k_db=3.0)
    ch = channel.MisoRaysFd(base.my_array.array_elements, base.my_standard_rx, delays, tap, amp, pts, ray_kind=kind, seed=77)
    link = mp_model.Link(mod_obj=mod, array_obj=base.my_array, std_rx_obj=base.my_standard_rx, chan_obj=ch,
                         noise_obj=copy.deepcopy(base.my_noise), rx_loc_var=10.0, n_err_min=10, bits_sent_max=1000, device=0)
    link.update_distortion(ibo_val_db=1.0)
    link.engine(reroll_chan=True)
    assert seen[-1]["args"][5] == "tdl" and seen[-1]["kw"]["chan_table"] is None and seen[-1]["tdl"] is None
    d, t, a, s, k = seen[-1]["rays"]
    np.testing.assert_array_equal(d, delays)
    np.testing.assert_array_equal(t, tap)
    np.testing.assert_array_equal(a, amp)
    np.testing.assert_array_equal(k, kind)
    np.testing.assert_allclose(s, ch.steer() / ch.ant_amp.max(), rtol=1e-15)
    assert np.abs(s).max() == pytest.approx(1.0, rel=1e-15)
    n = len(seen)
    link.engine(reroll_chan=True)
    assert len(seen) == n  # the same engine serves the next call
    link.engine(reroll_chan=False)
    assert seen[-1]["args"][5] == "table" and seen[-1]["rays"] is None
    np.testing.assert_array_equal(seen[-1]["kw"]["chan_table"], link.my_miso_chan.channel_mat_fd)


def test_sweep_parses_the_rays_channel(cpu_seam):
    import sweep
    ap = sweep.build_parser()
    for grid in ap._option_string_actions["--grid"].choices:
        args = ap.parse_args(["--grid", grid, "--channel", "rays", "--rays-clusters", "3", "--rays-per-cluster", "4",
                              "--rays-spread-deg", "2.5", "--rays-radius", "150", "--rays-k-db", "6"])
        assert (args.channel, args.rays_clusters, args.rays_per_cluster, args.rays_spread_deg, args.rays_radius,
                args.rays_k_db) == ("rays", 3, 4, 2.5, 150.0, 6.0)
    d = ap.parse_args(["--channel", "rays"])
    assert (d.rays_clusters, d.rays_per_cluster, d.rays_spread_deg, d.rays_radius, d.rays_k_db) == (None, 20, 5.0, 300.0, None)
    assert sweep.RESIDUAL_DISTORTION["rays"] is None
    base, _ = build_link(n_ant=4)
    tx, rx = base.my_array.array_elements, base.my_standard_rx
    ch = sweep.make_channel("rays", tx, rx, (5, 3, 1.5), (None, 4, 2.5, 150.0, None))
    assert str(ch) == "rays" and ch.delays.tolist() == [0, 3, 6, 9, 12] and np.all(np.bincount(ch.ray_tap) == 4)
    assert np.sum(ch.ray_amp ** 2) == pytest.approx(1.0)
    az = np.rad2deg(np.arctan2(ch.points[:, 1], ch.points[:, 0])).reshape(5, 4).mean(1)
    np.testing.assert_allclose(az, [18, 54, 90, 126, 162], atol=1e-9)  # evenly over the user's half-plane, y > 0
    np.testing.assert_allclose(np.hypot(ch.points[:, 0], ch.points[:, 1]), 150.0)
    assert np.all(ch.points[:, 2] == rx.cord_z)
    ck = sweep.make_channel("rays", tx, rx, (5, 3, 1.5), (2, 1, 0.0, 300.0, 6.0))
    assert ck.delays.tolist() == [0, 3] and ck.ray_kind.tolist() == [1, 0, 0]
    assert ck.points[0].tolist() == [rx.cord_x, rx.cord_y, rx.cord_z]
