"""Beam mode (mimo_engine_beam_points) on the GPU: the same counts as the plain run and the oracle,
per-trial rows of the five probe-field sums against the oracle-built reference (tests/beam_ref.py)
within a bound derived from the allowed errors of a chain output and of a probe-channel entry,
fixed-order totals, and the physics the beampattern must show.

Measured worst deviation-to-bound ratios per case: profiles/r11/beam/accuracy.md.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import beam_ref
from gpu_util import assert_counts_equal, engine_for
from oracle import refmath as rm
from oracle import sim
from utilities import circle_probes

pytestmark = pytest.mark.gpu

SEED = 7
N_TRIALS = 8
SNR64 = 25.0  # Es/N0 [dB] of the 64-QAM cases
RX = sim.SimConfig(n_ant=1, n_sc=4, n_fft=128, constel_size=4).rx_pos  # the default user


def probes_n(n):
    """n probes on the half circle through the user at its height; one probe: the user's direction."""
    angles = [45.0] if n == 1 else np.linspace(0.0, 180.0, n)
    return circle_probes(angles, math.hypot(RX[0], RX[1]), RX[2])


# the smallest shapes that reach every variant of the beam code: (config, iters, probes)
CASES = {
    # one-wave generic instance, cubic PA, an odd antenna count, a single probe
    "f128_toi": (dict(n_ant=5, n_sc=64, n_fft=128, constel_size=16, pa="toi", ibo_db=5.0, snr_db=20.0,
                      channel="rayleigh"), (0, 1), 1),
    # generic band that is not a multiple of a wave
    "f256_generic": (dict(n_ant=4, n_sc=100, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                          channel="rayleigh"), (0, 1), 37),
    # aligned, 4 slots, closed-form channel, fixed user; probes that do not fill the last block
    "f512_los": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                      channel="los", reroll=False), (0, 1), 65),
    # the CSI instance: X from the estimate
    "f512_csi": (dict(n_ant=8, n_sc=256, n_fft=512, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0,
                      channel="rayleigh", csi_eps=0.2), (0, 1), 37),
    # wave-split FFT, T 256, the MCNC loop's re-transmissions
    "f2048_mcnc": (dict(n_ant=4, n_sc=1024, n_fft=2048, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                        channel="rayleigh", receiver="mcnc"), (0, 1, 2), 37),
    # 8 slots, 16-point team
    "f4096_rapp": (dict(n_ant=2, n_sc=2048, n_fft=4096, constel_size=64, pa="rapp", p_hardness=3.0, ibo_db=3.0,
                        snr_db=SNR64, channel="rayleigh"), (0, 1), 37),
    # split FFT, T 512: the permuted frequency thread
    "f8192": (dict(n_ant=2, n_sc=4096, n_fft=8192, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64,
                   channel="rayleigh"), (0, 1), 37),
    # no PA: the field is the linear one
    "f256_nopa": (dict(n_ant=4, n_sc=128, n_fft=256, constel_size=64, pa="none", ibo_db=3.0, snr_db=SNR64,
                       channel="rayleigh"), (0,), 37),
}


@functools.lru_cache(maxsize=None)
def reference(name, ibo=None, first=0, n=N_TRIALS):
    kw, iters, nq = CASES[name]
    cfg = sim.SimConfig(**kw)
    if ibo is not None:
        cfg = dataclasses.replace(cfg, ibo_db=ibo)
    counts, rows, bounds = beam_ref.reference_rows(cfg, SEED, np.arange(first, first + n), iters, probes_n(nq))
    for a in (counts, rows, bounds):
        a.setflags(write=False)
    return cfg, counts, rows, bounds


def worst_ratio(label, rows_gpu, rows_ref, bounds):
    ratio = np.abs(np.asarray(rows_gpu) - rows_ref) / bounds
    worst = float(ratio.max())
    print(f"BEAM_RATIO case={label} worst={worst:.3e} per column="
          + ",".join(f"{v:.2e}" for v in ratio.reshape(-1, beam_ref.BEAM_FIXED).max(axis=0)))
    return worst


def assert_totals(total, rows):
    """A point's totals [n_probes, 5] are its per-trial rows' exact sums (fsum) to 1e-12: of the sum,
    and for Re / Im C, whose terms have either sign, of the sum of their magnitudes."""
    nq = rows.shape[1]
    tot = np.array([[math.fsum(rows[:, q, c]) for c in range(5)] for q in range(nq)])
    mag = np.array([[math.fsum(np.abs(rows[:, q, c])) for c in range(5)] for q in range(nq)])
    assert np.all(np.abs(total - tot) <= 1e-12 * mag), float(np.max(np.abs(total - tot) / mag))


@pytest.mark.parametrize("name", sorted(CASES))
def test_beam_rows_and_counts(name):
    cfg, ref_counts, ref_rows, bounds = reference(name)
    _, iters, nq = CASES[name]
    probes = probes_n(nq)
    eng = engine_for(cfg, precision="f64")
    err, bits, beam, per, per_beam = eng.beam(SEED, 0, N_TRIALS, iters, probes, per_trial=True)
    e_run, b_run, per_run = eng.run(SEED, 0, N_TRIALS, iters, per_trial=True)
    print(name, eng.describe(), "counts", per.sum(0))
    # the same trials, the same counts: the plain run's and the oracle's, exactly
    assert_counts_equal(per, per_run, f"{name}: beam vs run")
    assert_counts_equal(per, ref_counts, f"{name}: beam vs oracle")
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert per_beam.shape == ref_rows.shape == (N_TRIALS, nq, 5)
    assert np.all(np.isfinite(per_beam))
    worst = worst_ratio(name, per_beam, ref_rows, bounds)
    assert worst <= 1.0, f"{name}: per-trial row deviates {worst:.3g} x its bound"
    assert_totals(beam, per_beam)
    if cfg.receiver == "mcnc":
        # the MCNC re-transmissions stay out: the rows of the same system under CNC, bit for bit
        eng_c = engine_for(dataclasses.replace(cfg, receiver="cnc"), precision="f64")
        _, _, beam_c, _, per_beam_c = eng_c.beam(SEED, 0, N_TRIALS, iters, probes, per_trial=True)
        np.testing.assert_array_equal(per_beam_c, per_beam)
        np.testing.assert_array_equal(beam_c, beam)
        eng_c.close()
    if cfg.pa == "none":
        # Py_in = Px = Re C, Im C = 0, Py_oob = 0: each within the bounds of the cells involved
        px = per_beam[:, :, 2]
        assert np.all(np.abs(per_beam[:, :, 0] - px) <= bounds[:, :, 0] + bounds[:, :, 2])
        assert np.all(np.abs(per_beam[:, :, 3] - px) <= bounds[:, :, 3] + bounds[:, :, 2])
        assert np.all(np.abs(per_beam[:, :, 4]) <= bounds[:, :, 4])
        assert np.all(per_beam[:, :, 1] <= bounds[:, :, 1])
        assert np.all(bounds[:, :, 1] <= 1e-20 * px)  # ... which is nothing: no power off band
    eng.close()


def test_beam_points_rows_and_repeatability():
    """Case f256_generic's system at IBO 0 / 3 / 6 with 5 / 3 / 4 trials and distinct first trials, and a
    fourth point of one trial, in one call."""
    name = "f256_generic"
    _, iters, nq = CASES[name]
    probes = probes_n(nq)
    ibos, n_trials, first = (0.0, 3.0, 6.0, 3.0), (5, 3, 4, 1), (0, 16, 40, 60)
    refs = [reference(name, ibo, f, n) for ibo, f, n in zip(ibos, first, n_trials)]
    eng = engine_for(refs[1][0], precision="f64")
    points = []
    for r in refs:
        e = engine_for(r[0], precision="f64")
        points.append(dict(e.point_kw))
        e.close()
    seeds = [SEED] * 4
    err, bits, beam, per, per_beam = eng.beam_points(points, seeds, first, n_trials, iters, probes, per_trial=True)
    e_run, b_run, per_run = eng.run_points(points, seeds, first, n_trials, iters, per_trial=True)
    np.testing.assert_array_equal(err, e_run)
    np.testing.assert_array_equal(bits, b_run)
    assert_counts_equal(per, per_run, "beam_points vs run_points")
    assert_counts_equal(per, np.concatenate([r[1] for r in refs]), "beam_points vs oracle")
    worst = worst_ratio("multipoint", per_beam, np.concatenate([r[2] for r in refs]),
                        np.concatenate([r[3] for r in refs]))
    assert worst <= 1.0
    off = np.concatenate(([0], np.cumsum(n_trials)))
    for i in range(4):
        own = per_beam[off[i]:off[i + 1]]
        assert_totals(beam[i], own)
        # every point's rows are those of a single-point call, bit for bit
        _, _, b1, _, pb1 = eng.beam(seeds[i], first[i], n_trials[i], iters, probes, per_trial=True, point=points[i])
        np.testing.assert_array_equal(pb1, own)
        assert_totals(b1, own)
    # a second identical call: bit-identical totals and rows
    _, _, beam2, _, per_beam2 = eng.beam_points(points, seeds, first, n_trials, iters, probes, per_trial=True)
    np.testing.assert_array_equal(beam2, beam)
    np.testing.assert_array_equal(per_beam2, per_beam)
    eng.close()


def test_beam_rows_do_not_depend_on_the_launch_splitting(monkeypatch):
    """MIMO_MAX_LAUNCH_TRIALS = 3, then a beam buffer that holds two trials' cells (32 n_ant n_fft
    bytes each): the rows and counts are those of the single launch."""
    cfg = sim.SimConfig(n_ant=4, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64)
    probes = probes_n(9)
    eng = engine_for(cfg, precision="f64")
    n = 11
    err, _, beam, per, pb = eng.beam(SEED, 0, n, (0, 1), probes, per_trial=True)
    np.testing.assert_array_equal(err, per.sum(0))
    assert np.all(pb[:, :, 0] > 0)
    for var, val in (("MIMO_MAX_LAUNCH_TRIALS", "3"), ("MIMO_BEAM_BUFFER_BYTES", str(2 * 32 * 4 * 256 + 100))):
        monkeypatch.setenv(var, val)
        err3, _, beam3, per3, pb3 = eng.beam(SEED, 0, n, (0, 1), probes, per_trial=True)
        monkeypatch.delenv(var)
        np.testing.assert_array_equal(pb3, pb)
        np.testing.assert_array_equal(per3, per)
        np.testing.assert_array_equal(err3, err)
        assert_totals(beam3, pb)
    eng.close()


def test_one_antenna_beam_is_its_spectrum_times_the_path_loss():
    """A = 1: |R_q[k]|^2 = att_q[k]^2 |Y[k]|^2, so the beam totals are the engine's own spectrum
    totals weighted by the squared free-space attenuation."""
    cfg = sim.SimConfig(n_ant=1, n_sc=128, n_fft=256, constel_size=64, pa="softlim", ibo_db=3.0, snr_db=SNR64)
    probes = probes_n(9)
    eng = engine_for(cfg, precision="f64")
    _, _, beam, _, _ = eng.beam(SEED, 0, N_TRIALS, (0,), probes)
    _, _, spec, _, _ = eng.spectrum(SEED, 0, N_TRIALS, (0,))
    eng.close()
    for i, q in enumerate(probes):
        att = rm.fspl_matrix(cfg.tx_pos, q, cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)[0]
        want = float((att ** 2 * spec[:cfg.n_fft]).sum())
        assert abs(beam[i, 0] + beam[i, 1] - want) <= 1e-11 * want, (i, beam[i, 0] + beam[i, 1], want)


@pytest.mark.parametrize("ibo", (0.0, 3.0))
def test_los_physics_on_the_device(ibo):
    """tests/beam_ref.py's LoS physics system (tests/test_beam_host.py checks its reference): the same
    argmax, pooled figures within 1e-9 of the reference's."""
    import _engine
    host = beam_ref
    cfg, ref_rows = host.pooled_reference("los", ibo)
    ref = _engine.BeamStats(ref_rows.sum(0), host.PHYS_TRIALS)
    eng = engine_for(cfg, precision="f64")
    _, _, beam, _, _ = eng.beam(host.PHYS_SEED, 0, host.PHYS_TRIALS, (0,), host.phys_probes())
    eng.close()
    gpu = _engine.BeamStats(beam, host.PHYS_TRIALS)
    for which in ("signal", "distortion", "power_oob"):
        g, r = getattr(gpu, which), getattr(ref, which)
        print(f"BEAM_PHYS ibo={ibo} {which}: worst relative deviation {np.max(np.abs(g - r) / r):.3e}, "
              f"directivity gpu {gpu.directivity(which):.6f} oracle {ref.directivity(which):.6f}")
        assert int(np.argmax(g)) == int(np.argmax(r)) == host.USER
        assert np.all(np.abs(g - r) <= 1e-9 * r), which
        assert abs(gpu.directivity(which) - ref.directivity(which)) <= 1e-9 * ref.directivity(which)
    assert np.all(np.abs(gpu.gain - ref.gain) <= 1e-9 * np.abs(ref.gain))


def test_link_beampattern_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    import _engine
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM
    link.set_snr(14.0)
    probes = probes_n(19)
    st = link.beampattern(True, [11, 22, 33], N_TRIALS, probes)
    eng = link.engine()
    _, _, beam, _, _ = eng.beam(_seed64([11, 22, 33]), 0, N_TRIALS, [0], probes, point=link.point_params())
    np.testing.assert_array_equal(st.rows, beam)
    assert (st.n_probes, st.n_trials) == (19, N_TRIALS)
    ref = _engine.BeamStats(beam)
    np.testing.assert_array_equal(st.signal, ref.signal)
    np.testing.assert_array_equal(st.sdr_db, ref.sdr_db)
    assert np.all(st.power_inband > 0) and np.all(st.distortion > 0)
    # through beampattern_points at two IBOs: point 0 is the call above
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.beampattern_points(True, [[11, 22, 33], [5]], [p0, p1], N_TRIALS, probes)
    np.testing.assert_array_equal(both[0].rows, st.rows)
    assert both[1].n_probes == 19


def test_the_largest_probe_list():
    """4,096 probes (MIMO_BEAM_MAX_PROBES: 512 blocks of probes per tile of trials) on the smallest
    system: rows within the bound, totals their sums."""
    cfg = sim.SimConfig(n_ant=2, n_sc=64, n_fft=128, constel_size=16, pa="softlim", ibo_db=3.0, snr_db=20.0)
    probes = probes_n(4096)
    counts, rows, bounds = beam_ref.reference_rows(cfg, SEED, np.arange(3), (0,), probes)
    eng = engine_for(cfg, precision="f64")
    _, _, beam, per, per_beam = eng.beam(SEED, 0, 3, (0,), probes, per_trial=True)
    eng.close()
    assert_counts_equal(per, counts, "4096 probes vs oracle")
    assert worst_ratio("max_probes", per_beam, rows, bounds) <= 1.0
    assert_totals(beam, per_beam)
