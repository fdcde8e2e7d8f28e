"""Beam mode on a machine without a GPU: the width helper, the host-side argument checks of
mimo_engine_beam_points (no HIP call before them), BeamStats arithmetic on hand-made rows,
utilities.circle_probes, sweep.beam_vs_angle with its CSV writer against a fake link, and the
physics of the oracle-built reference (tests/beam_ref.py) that the GPU tests compare against."""
import ctypes
import math
import warnings

import numpy as np
import pytest

import _engine
import beam_ref
import fake_beam_link as fbl
import spectrum_ref
from oracle import refmath as rm
from oracle import sim

_dp = ctypes.POINTER(ctypes.c_double)
_u64 = ctypes.POINTER(ctypes.c_uint64)


def _engine_handle(precision=0):
    lib = _engine.lib()
    tx = np.array([[-0.1, 0.0, 15.0], [-0.05, 0.0, 15.0], [0.05, 0.0, 15.0], [0.1, 0.0, 15.0]])
    fr = np.full(512, 3.5e9)
    c = _engine.MimoConfig(n_ant=4, n_sub_carr=256, n_fft=512, constel_size=16, cp_len=16, channel_kind=1,
                           receiver_kind=1, device=-1, rx_loc_var=10.0, reroll_chan=1, precision=precision,
                           tx_pos=tx.ctypes.data_as(_dp), carrier_freqs=fr.ctypes.data_as(_dp))
    h = lib.mimo_engine_create(ctypes.byref(c))
    assert h
    return lib, h, (tx, fr)


GOOD_PROBES = np.array([[212.0, 212.0, 1.5], [0.0, 300.0, 1.5]])


def _beam(lib, h, probes=GOOD_PROBES, n_probes=None, out="own", iters=(0,)):
    """-> (rc, message, beam_out): one point of 8 trials; ``probes`` None passes a null pointer,
    ``out`` None a null beam_out."""
    pt = _engine.Engine.make_point(3.0, 20.0, 10.0, "softlim", sat_pow=1.0, cnc_sat_pow=1.0, cnc_alpha=0.9)
    it = np.asarray(iters, np.int32)
    one = lambda v: np.asarray([v], np.uint64)  # noqa: E731
    seeds, first, n = one(1), one(0), one(8)
    err = np.zeros(8, np.uint64)
    bits = np.zeros(8, np.uint64)
    pr = None if probes is None else np.ascontiguousarray(probes, np.float64)
    nq = (0 if pr is None else len(pr)) if n_probes is None else n_probes
    beam = None if out is None else np.full((max(1, min(nq, 8)), 5), 7.0)
    rc = lib.mimo_engine_beam_points(h, 1, ctypes.byref(pt), seeds.ctypes.data_as(_u64), first.ctypes.data_as(_u64),
                                     n.ctypes.data_as(_u64), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(it),
                                     0, err.ctypes.data_as(_u64), bits.ctypes.data_as(_u64), None,
                                     pr.ctypes.data_as(_dp) if pr is not None else None, nq,
                                     beam.ctypes.data_as(_dp) if beam is not None else None, None)
    return rc, lib.mimo_last_error().decode(), beam


def test_beam_width():
    lib = _engine.lib()
    assert _engine.BEAM_FIXED == 5
    for n in (1, 37, 181, 4096):
        assert lib.mimo_beam_width(n) == 5 * n
    for bad in (0, -3, 4097):
        assert lib.mimo_beam_width(bad) == -1  # MIMO_EINVAL
        assert "n_probes" in lib.mimo_last_error().decode()


def test_beam_rejects_float32_engine_before_any_hip_call():
    lib, h, keep = _engine_handle(precision=1)
    rc, msg, beam = _beam(lib, h)
    assert rc == -1 and "float64" in msg and "beam" in msg, (rc, msg)
    assert np.all(beam == 7.0)  # nothing added
    lib.mimo_engine_destroy(h)


@pytest.mark.parametrize("kw,msg", [
    (dict(probes=None, n_probes=2), "null probes"),
    (dict(out=None), "null beam_out"),
    (dict(n_probes=0), "n_probes must be in [1, 4096]"),
    (dict(n_probes=4097), "n_probes must be in [1, 4096]"),
    (dict(n_probes=-1), "n_probes must be in [1, 4096]"),
    (dict(probes=[[212.0, 212.0, 1.5], [0.0, float("nan"), 1.5]]), "probe 1 is not finite"),
    (dict(probes=[[float("inf"), 212.0, 1.5]]), "probe 0 is not finite"),
    (dict(probes=[[212.0, 212.0, 1.5], [0.0, 300.0, -float("inf")]]), "probe 1 is not finite"),
    (dict(probes=[[212.0, 212.0, 1.5], [0.05, 0.0, 15.0]]), "probe 1 coincides with antenna 2"),
    (dict(iters=(2, 1)), "sorted and unique"),
])
def test_beam_rejects_bad_arguments_before_any_hip_call(kw, msg):
    lib, h, keep = _engine_handle()
    rc, got, beam = _beam(lib, h, **kw)
    assert rc == -1 and msg in got, (rc, got)
    if beam is not None:
        assert np.all(beam == 7.0)
    lib.mimo_engine_destroy(h)


def test_beam_rejects_a_system_of_which_one_trial_does_not_fit_the_buffer(monkeypatch):
    """One trial's cells are 32 n_ant n_fft bytes (65,536 here); a buffer of one byte less holds none."""
    lib, h, keep = _engine_handle()
    monkeypatch.setenv("MIMO_BEAM_BUFFER_BYTES", str(32 * 4 * 512 - 1))
    rc, msg, beam = _beam(lib, h)
    assert rc == -1 and "do not fit the beam buffer" in msg and "65536" in msg, (rc, msg)
    assert np.all(beam == 7.0)
    lib.mimo_engine_destroy(h)


# ---------------------------------------------------------------- BeamStats
# probe 0: a linear array towards it; probe 1: gain 0.75 - 0.5j; probe 2: nothing arrives in band
HAND = np.array([[20.0, 0.0, 20.0, 20.0, 0.0],
                 [16.0, 1.0, 16.0, 12.0, -8.0],
                 [0.0, 0.5, 0.0, 0.0, 0.0]])


def test_beam_stats_exact_values():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st = _engine.BeamStats(HAND, n_trials=2)
        assert (st.n_probes, st.n_trials) == (3, 2)
        np.testing.assert_array_equal(st.rows, HAND)
        np.testing.assert_array_equal(st.power_inband, [20.0, 16.0, 0.0])
        np.testing.assert_array_equal(st.power_oob, [0.0, 1.0, 0.5])
        np.testing.assert_array_equal(st.input_power, [20.0, 16.0, 0.0])
        np.testing.assert_array_equal(st.c, [20.0, complex(12.0, -8.0), 0.0])
        assert st.gain[0] == 1.0 and st.gain[1] == complex(0.75, -0.5) and np.isinf(st.gain[2])
        # |C|^2 / Px = 208 / 16 = 13 of the 16 in band at probe 1
        np.testing.assert_array_equal(st.signal[:2], [20.0, 13.0])
        np.testing.assert_array_equal(st.distortion[:2], [0.0, 3.0])
        assert st.sdr_db[0] == np.inf
        assert st.sdr_db[1] == pytest.approx(10 * np.log10(13.0 / 3.0), abs=1e-12)
        assert st.directivity("power_oob") == 1.0 / 0.5
        assert st.directivity("input_power") == 20.0 / 12.0
        two = _engine.BeamStats(HAND[:2])
        assert two.n_trials is None
        assert two.directivity("signal") == 20.0 / 16.5
        assert two.directivity("distortion") == 2.0
        np.testing.assert_allclose(two.pattern_db("signal"), 10 * np.log10([20.0 / 16.5, 13.0 / 16.5]), rtol=1e-13)
        np.testing.assert_allclose(two.pattern_db("power_oob", ref=2.0), [-np.inf, 10 * np.log10(0.5)], rtol=1e-13)
    with pytest.raises(ValueError, match="which"):
        st.directivity("psd")
    for bad in (np.ones(5), np.ones((2, 4)), np.ones((0, 5))):
        with pytest.raises(ValueError, match="n_probes, 5"):
            _engine.BeamStats(bad)


def test_beam_stats_pooling_is_the_row_sum():
    rng = np.random.default_rng(5)
    rows = rng.uniform(1.0, 2.0, (3, 7, 5))
    parts = [_engine.BeamStats(rows[i], n_trials=i + 1) for i in range(3)]
    pooled = parts[0] + parts[1] + parts[2]
    direct = _engine.BeamStats((rows[0] + rows[1]) + rows[2])
    np.testing.assert_array_equal(pooled.rows, direct.rows)
    assert pooled.n_trials == 6
    np.testing.assert_array_equal(pooled.signal, direct.signal)
    np.testing.assert_array_equal(pooled.gain, direct.gain)
    assert (parts[0] + _engine.BeamStats(rows[1])).n_trials is None
    with pytest.raises(ValueError, match="different probe lists"):
        parts[0] + _engine.BeamStats(np.ones((6, 5)))


def test_circle_probes():
    from utilities import circle_probes
    p = circle_probes([0.0, 90.0, 180.0, 45.0], 2.0, 1.5)
    assert p.shape == (4, 3) and p.dtype == np.float64
    np.testing.assert_allclose(p, [[2.0, 0.0, 1.5], [0.0, 2.0, 1.5], [-2.0, 0.0, 1.5],
                                   [math.sqrt(2.0), math.sqrt(2.0), 1.5]], atol=1e-15)
    th = np.deg2rad(np.arange(0.0, 181.0, 5.0))
    q = circle_probes(np.arange(0.0, 181.0, 5.0), 300.0)
    np.testing.assert_array_equal(q, np.stack([300.0 * np.cos(th), 300.0 * np.sin(th), np.zeros(37)], axis=1))
    assert circle_probes(30.0, 1.0).shape == (1, 3)


def test_beam_vs_angle_and_csv_writer(tmp_path):
    import sweep
    from utilities import circle_probes, read_from_csv, save_to_csv
    link = fbl.FakeBeamLink()
    ibos = np.array([0.0, 3.0])
    angles = np.array([0.0, 45.0, 90.0, 135.0])
    probes, stats = sweep.beam_vs_angle(link, angles, ibos, 5, seed=11)
    assert len(link.calls) == 1  # every point in one call
    call = link.calls[0]
    assert call["ibos"] == [0.0, 3.0] and call["n_trials"] == 5 and call["reroll_chan"] is True
    assert call["seeds"] == [sweep.point_seed(11, i) for i in range(2)]
    # the circle through the user, at its height
    np.testing.assert_array_equal(probes, circle_probes(angles, 5.0, 1.5))
    np.testing.assert_array_equal(call["probes"], probes)
    for ibo, st in zip(ibos, stats):
        np.testing.assert_array_equal(st.rows, fbl.fake_rows(ibo, 5, 4))
    save_to_csv(sweep.beam_vs_angle_rows(angles, stats), "beam", directory=str(tmp_path))
    back = np.asarray(read_from_csv("beam", directory=str(tmp_path)))
    assert back.shape == (4, 1 + 3 * 2)
    np.testing.assert_array_equal(back[:, 0], angles)
    sig = (2.0 + np.arange(4)) ** 2 / 4.0  # per trial; mean 54 / 16
    for j, ibo in enumerate(ibos):
        np.testing.assert_allclose(back[:, 1 + 3 * j], 10 * np.log10(sig / sig.mean()), rtol=1e-12)
        np.testing.assert_allclose(back[:, 2 + 3 * j], 10 * np.log10(0.5 / (1 + ibo) / sig.mean()), rtol=1e-12)
        np.testing.assert_allclose(back[:, 3 + 3 * j], 10 * np.log10((1.0 + np.arange(4)) / 100.0 / sig.mean()),
                                   rtol=1e-12)
    # an explicit circle
    probes2, _ = sweep.beam_vs_angle(link, angles, ibos[:1], 2, radius=10.0, z=0.0)
    np.testing.assert_array_equal(probes2, circle_probes(angles, 10.0, 0.0))


# ---------------------------------------------------------------- physics of the reference
PHYS, PHYS_SEED, PHYS_TRIALS = beam_ref.PHYS, beam_ref.PHYS_SEED, beam_ref.PHYS_TRIALS
PHYS_ANGLES, USER = beam_ref.PHYS_ANGLES, beam_ref.USER
phys_probes, pooled_reference = beam_ref.phys_probes, beam_ref.pooled_reference


@pytest.mark.parametrize("ibo", (0.0, 3.0))
def test_los_beamforms_signal_distortion_and_oob_towards_the_user(ibo):
    cfg, rows = pooled_reference("los", ibo)
    st = _engine.BeamStats(rows.sum(0), PHYS_TRIALS)
    assert PHYS_ANGLES[USER] == 45.0
    d = {w: st.directivity(w) for w in ("signal", "distortion", "power_oob")}
    alpha = float(rm.calc_alpha(ibo))
    print(f"BEAM_PHYS los ibo={ibo}: directivity {d} |gain| at the user {abs(st.gain[USER]):.4f} alpha {alpha:.4f}")
    for which in d:
        assert int(np.argmax(getattr(st, which))) == USER, which
        assert d[which] >= 0.9 * cfg.n_ant, (which, d[which])
    assert abs(abs(st.gain[USER]) - alpha) <= 0.015 * alpha, (abs(st.gain[USER]), alpha)


@pytest.mark.parametrize("ibo", (0.0, 3.0))
def test_rayleigh_radiates_all_three_evenly(ibo):
    _, rows = pooled_reference("rayleigh", ibo)
    st = _engine.BeamStats(rows.sum(0), PHYS_TRIALS)
    d = {w: st.directivity(w) for w in ("signal", "distortion", "power_oob")}
    print(f"BEAM_PHYS rayleigh ibo={ibo}: directivity {d}")
    for which, v in d.items():
        assert v <= 1.1, (which, v)


def test_a_linear_array_radiates_its_input():
    _, rows = pooled_reference("los", 3.0, pa="none")
    px = rows[:, :, 2]
    assert np.all(px > 0)
    assert np.all(np.abs(rows[:, :, 0] - px) <= 1e-12 * px)
    assert np.all(np.abs(rows[:, :, 3] - px) <= 1e-12 * px)
    assert np.all(np.abs(rows[:, :, 4]) <= 1e-12 * px)
    assert np.all(rows[:, :, 1] <= 1e-12 * px)


def test_one_antenna_radiates_its_spectrum_times_the_path_loss():
    cfg = sim.SimConfig(**dict(PHYS, n_ant=1, channel="los", ibo_db=3.0))
    probes = phys_probes()[::6]
    trials = np.arange(4)
    _, rows, _ = beam_ref.reference_rows(cfg, PHYS_SEED, trials, (0,), probes, bounds=False)
    _, spec = spectrum_ref.reference_rows(cfg, PHYS_SEED, trials, (0,))
    psd = spec[:, :cfg.n_fft]
    for i, q in enumerate(probes):
        att = rm.fspl_matrix(cfg.tx_pos, q, cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)[0]
        want = (att ** 2 * psd).sum(1)
        np.testing.assert_allclose(rows[:, i, 0] + rows[:, i, 1], want, rtol=1e-12, atol=0)
