"""The ray-cluster channel on the GPU: the fine seam mimo_rays_channels against the long-double
reference (tests/rays_ref.py) stage by stage, its exact anchors and streams, the engine's generator
against the seam (a bank engine holding the seam's matrices must give the same bits), the two
profile setters on one engine, a rays engine's per-trial counts against the oracle run on the seam's
channels, and where an array's distortion goes when one specular ray points the channel somewhere.
"""
import dataclasses

import numpy as np
import pytest

import _engine
import rays_ref
import tdl_ref
from gpu_util import PRECISIONS, assert_counts_equal, assert_f32_counts_close, engine_for
from oracle import refmath as rm
from oracle import sim
from utilities import circle_probes, scatterer_steering

pytestmark = pytest.mark.gpu

FACTOR = 16.0  # tests/test_gpu_tdl.py test_seam_accuracy's yardstick factor
HIGH_SEED = 0xFEDCBA9876543210
ITERS = (0, 1, 2)


def layout(counts):
    """ray_tap of a profile with counts[l] rays in tap l."""
    return np.repeat(np.arange(len(counts)), counts)


def spread_delays(n_taps, n_fft):
    """n_taps ascending delays from 0 up to n_fft - 1, unevenly spaced (one tap: delay 5)."""
    if n_taps == 1:
        return np.array([5])
    inner = np.random.default_rng(n_fft).choice(np.arange(1, n_fft - 1), n_taps - 2, replace=False)
    return np.sort(np.concatenate(([0], inner, [n_fft - 1]))).astype(np.int64)


def profile(counts, n_fft, n_ant, mixed):
    """delays, ray_tap, ray_amp, steer (complex, non-unit), ray_kind (every third ray specular, or None)."""
    ray_tap = layout(counts)
    R = ray_tap.size
    rng = np.random.default_rng(R * 131 + n_ant)
    amp = 0.25 + rng.random(R)
    steer = (0.5 + rng.random((n_ant, R))) * np.exp(2j * np.pi * rng.random((n_ant, R)))
    kind = (np.arange(R) % 3 == 1).astype(np.uint8) if mixed else None
    return spread_delays(len(counts), n_fft), ray_tap, amp, steer, kind


# (rays per tap, n_fft, n_ant, n, first_trial, seed, mixed kinds): the issue's extremes together, and the two
# sizes of the dynamic LDS block at which the launch changes (R 1024 beside W: 48 KiB at F 2048, 80 KiB at 4096)
SEAM_CASES = [([1], 128, 1, 1, 0, 1, False), ([1024], 128, 3, 2, 3, 77, True), ([1] * 64, 8192, 3, 5, 11, 5, False),
              ([1, 300, 2, 61], 512, 2, 3, 7, 9, True), ([2, 3], 128, 2, 5, 2 ** 32 - 2, 21, True),
              ([4, 1, 7], 256, 3, 2, 1, HIGH_SEED, True), ([1000, 24], 2048, 2, 1, 0, 3, True),
              ([24, 1000], 4096, 2, 2, 5, 4, True)]


def case_id(c):
    counts = c[0]
    return f"L{len(counts)}-R{sum(counts)}-F{c[1]}-A{c[2]}-n{c[3]}"


@pytest.mark.parametrize("counts,F,A,n,first,seed,mixed", SEAM_CASES, ids=[case_id(c) for c in SEAM_CASES])
def test_seam_accuracy(counts, F, A, n, first, seed, mixed):
    delays, ray_tap, amp, steer, kind = profile(counts, F, A, mixed)
    L, R = len(counts), ray_tap.size
    h, g, c = _engine.rays_channels(delays, ray_tap, amp, steer, F, seed, first, n, ray_kind=kind, taps=True, gains=True)
    assert h.shape == (n, A, F) and g.shape == (n, A, L) and c.shape == (n, R)
    # gains: error relative to |c| against 16 times NumPy's own on the same elements (on at least 257)
    n_y = max(n, -(-257 // R))
    cy = c if n_y == n else _engine.rays_channels(delays, ray_tap, amp, steer, F, seed, first, n_y, ray_kind=kind,
                                                 gains=True)[1]
    np.testing.assert_array_equal(cy[:n], c)
    ty = [first + j for j in range(n_y)]
    ld = rays_ref.ld_gains(amp, seed, ty, kind)
    e_np = float(np.max(np.abs(rays_ref.np_gains(amp, seed, ty, kind) - ld) / np.abs(ld)))
    err = float(np.max(np.abs(cy - ld) / np.abs(ld)))
    print(f"gains: device {err:.3e}, NumPy {e_np:.3e} (bound {FACTOR * e_np:.3e}) over {cy.size} elements")
    assert e_np > 0 and err <= FACTOR * e_np
    # taps: against the long-double sum of the device's own gains, an order-independent rounding bound
    ref_g = rays_ref.ld_taps_of(c, ray_tap, steer)
    mass = np.einsum("nr,ar,rl->nal", np.abs(c), np.abs(steer), (ray_tap[:, None] == np.arange(L)[None, :]).astype(float))
    bound_g = (np.asarray(counts)[None, None, :] + 8) * 2.0 ** -53 * mass
    dg = g - ref_g
    worst_g = float(np.max(np.maximum(np.abs(dg.real), np.abs(dg.imag)) / bound_g))
    print(f"taps: worst error / bound {worst_g:.3f}")
    assert np.all(np.abs(dg.real) <= bound_g) and np.all(np.abs(dg.imag) <= bound_g)
    # transform: H against the long-double DFT of the device's own taps
    ref = tdl_ref.ld_response(g, delays, F)
    bound = (L + 8) * 2.0 ** -53 * np.sum(np.abs(g), axis=-1, keepdims=True)
    dev = h - ref
    worst = float(np.max(np.maximum(np.abs(dev.real), np.abs(dev.imag)) / bound))
    print(f"transform: worst error / bound {worst:.3f}")
    assert np.all(np.abs(dev.real) <= bound) and np.all(np.abs(dev.imag) <= bound)
    for v in (h, g, c):
        assert np.all(np.isfinite(v.view(np.float64)))
    if kind is not None:  # a specular ray's modulus is its amplitude
        spec = kind == 1
        np.testing.assert_allclose(np.abs(c[:, spec]), np.broadcast_to(amp[spec], (n, spec.sum())), rtol=4 * 2.0 ** -52)
    # trial indices are taken mod 2^32
    if first + n > 2 ** 32:
        k = 2 ** 32 - first
        np.testing.assert_array_equal(h[k:], _engine.rays_channels(delays, ray_tap, amp, steer, F, seed, 0, n - k,
                                                                  ray_kind=kind))


@pytest.mark.parametrize("delays", [[0], [0, 3, 64, 127]], ids=["flat", "L4"])
def test_exact_anchor(delays):
    """steer = 1 + 0j, one diffuse ray per tap: the taps are the gains and every antenna's row of H is
    the same, bit for bit; one tap at delay 0 is flat at the gain."""
    L, A = len(delays), 3
    h, g, c = _engine.rays_channels(delays, np.arange(L), np.linspace(0.5, 1.5, L), np.ones((A, L), complex), 128, 11, 4, 3,
                                    taps=True, gains=True)
    assert np.all(c.real != 0) and np.all(c.imag != 0)
    np.testing.assert_array_equal(g.view(np.float64), np.broadcast_to(c[:, None, :], g.shape).copy().view(np.float64))
    for a in range(1, A):
        np.testing.assert_array_equal(h[:, a].view(np.float64), h[:, 0].view(np.float64))
    if L == 1:
        np.testing.assert_array_equal(h.real, np.broadcast_to(c.real[:, :, None], h.shape))
        np.testing.assert_array_equal(h.imag, np.broadcast_to(c.imag[:, :, None], h.shape))
    else:
        assert len(np.unique(h[0, 0])) > 1


def test_seam_streams_are_distinct_and_repeatable():
    args = ([0, 3], [0, 0, 1], [1.0, 1.0, 1.0], np.ones((2, 3), complex), 128)

    def gains(seed, t0, n):
        return _engine.rays_channels(*args, seed, t0, n, gains=True)[1]

    base = gains(0x1234, 4, 2)
    vals = [base[0, 0], base[0, 1], base[0, 2], base[1, 0]]  # then: ray (twice), trial changed
    vals.append(gains(0x1235, 4, 2)[0, 0])              # seed, low word
    vals.append(gains(0x1234 | (1 << 40), 4, 2)[0, 0])  # seed, high word
    assert len(set(vals)) == len(vals) and len({v.real for v in vals}) == len(vals)
    np.testing.assert_array_equal(gains(0x1234, 4, 2), base)
    np.testing.assert_array_equal(gains(0x1234, 5, 1)[0], base[1])
    # the TDL taps' stream is another one: a diffuse ray is not tap 0 of antenna 0
    tdl_tap = _engine.tdl_channels([0], [1.0], 1, 128, 0x1234, 4, 1, taps=True)[1][0, 0, 0]
    assert tdl_tap != base[0, 0]


# ---------------------------------------------------------------- the engine's generator
def rays_cfg(A, S, F, receiver="cnc", M=16):
    return sim.SimConfig(A, S, F, M, ibo_db=1.0, snr_db=14.0, channel="tdl", receiver=receiver)


def rays_profile_for(A, F):
    """3 taps with 2, 5 and 1 rays, one of them specular, complex non-unit steering."""
    rng = np.random.default_rng(A * 1000 + F)
    steer = (0.4 + 0.6 * rng.random((A, 8))) * np.exp(2j * np.pi * rng.random((A, 8)))
    amp = np.array([0.5, 0.4, 0.3, 0.25, 0.2, 0.3, 0.2, 0.35])
    kind = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint8)
    return np.array([0, 2, F // 4 + 1]), layout([2, 5, 1]), amp, steer, kind


def rays_engine(cfg, prec):
    eng = engine_for(cfg, precision=prec)
    eng.set_rays(*rays_profile_for(cfg.n_ant, cfg.n_fft))
    assert "ch=4" in eng.describe()  # the table instances
    return eng


def seam_h(cfg, seed, t0, n):
    d, rt, amp, steer, kind = rays_profile_for(cfg.n_ant, cfg.n_fft)
    return _engine.rays_channels(d, rt, amp, steer, cfg.n_fft, seed, t0, n, ray_kind=kind)


def bank_of_seam(cfg, prec, seed, t0, n):
    """A bank engine holding the seam's matrices of trials t0 .. t0 + n - 1, ordered by trial mod n."""
    h = seam_h(cfg, seed, t0, n)
    bank = np.empty_like(h)
    for j in range(n):
        bank[(t0 + j) % n] = h[j]
    eng = engine_for(dataclasses.replace(cfg, channel="table", table_h=bank[0], reroll=False), precision=prec)
    eng.set_channel_bank(bank)
    return eng


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("receiver", ["cnc", "mcnc"])
@pytest.mark.parametrize("A,S,F", [(8, 256, 512), (3, 100, 128)])
def test_engine_generator_equals_the_seam(A, S, F, receiver, prec):
    cfg = rays_cfg(A, S, F, receiver)
    eng = rays_engine(cfg, prec)
    n = 6
    per = {}
    for t0, seed in ((0, 31), (7, 31), (3, 32)):
        _, _, per[t0, seed] = eng.run(seed, t0, n, ITERS, True, per_trial=True)
        ref = bank_of_seam(cfg, prec, seed, t0, n)
        _, _, want = ref.run(seed, t0, n, ITERS, True, per_trial=True)
        ref.close()
        np.testing.assert_array_equal(per[t0, seed], want, err_msg=f"t0 {t0} seed {seed}")
    assert eng.chan_kernel_ms > 0 and eng.kernel_ms > 0
    assert np.any(per[0, 31] != per[7, 31])
    # two points with different seeds in one launch: each block's entry is its own (seed, trial)'s
    _, _, both = eng.run_points([eng.point_kw, eng.point_kw], [31, 32], [7, 3], [n, n], ITERS, True, per_trial=True)
    np.testing.assert_array_equal(both, np.concatenate([per[7, 31], per[3, 32]]))
    eng.close()


def test_engine_generator_equals_the_seam_in_soft_mode():
    cfg = rays_cfg(4, 100, 256, M=64)
    eng, ref = rays_engine(cfg, "f64"), bank_of_seam(cfg, "f64", 31, 7, 5)
    got = eng.soft(31, 7, 5, ITERS, 8.0, True, per_trial=True)
    want = ref.soft(31, 7, 5, ITERS, 8.0, True, per_trial=True)
    eng.close()
    ref.close()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"soft output {k}")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_last_setter_wins(prec):
    cfg = rays_cfg(3, 100, 128)
    tdl = (np.array([0, 2, 5]), np.array([0.5, 0.3, 0.2]), np.linspace(0.5, 1.0, 3))
    rays = rays_profile_for(3, 128)

    def counts(*setters):
        eng = engine_for(cfg, precision=prec)
        for kind in setters:
            eng.set_tdl(*tdl) if kind == "tdl" else eng.set_rays(*rays)
        _, _, per = eng.run(31, 2, 8, ITERS, True, per_trial=True)
        eng.close()
        return per

    fresh_tdl, fresh_rays = counts("tdl"), counts("rays")
    assert np.any(fresh_tdl != fresh_rays)
    np.testing.assert_array_equal(counts("rays", "tdl"), fresh_tdl)
    np.testing.assert_array_equal(counts("tdl", "rays"), fresh_rays)
    # ... and between two runs of one engine
    eng = engine_for(cfg, precision=prec)
    eng.set_rays(*rays)
    _, _, a = eng.run(31, 2, 8, ITERS, True, per_trial=True)
    eng.set_tdl(*tdl)
    _, _, b = eng.run(31, 2, 8, ITERS, True, per_trial=True)
    eng.set_rays(*rays)
    _, _, c = eng.run(31, 2, 8, ITERS, True, per_trial=True)
    eng.close()
    np.testing.assert_array_equal(a, fresh_rays)
    np.testing.assert_array_equal(b, fresh_tdl)
    np.testing.assert_array_equal(c, fresh_rays)


# ---------------------------------------------------------------- the oracle on the seam's channels
@pytest.mark.parametrize("prec", PRECISIONS)
def test_rays_engine_vs_oracle(prec):
    """A 8, S 256, F 512, CNC iterations 0, 1 and 2, 16 trials: oracle.sim.run_trial with
    channel="table" and table_h the seam's H of the trial, labels and noise from sim.draws.
    float64: exact; float32: the project's float32 criterion (gpu_util.assert_f32_counts_close)."""
    cfg = rays_cfg(8, 256, 512)
    seed, n = 2137, 16
    h = seam_h(cfg, seed, 0, n)
    dr = sim.draws(cfg, seed, np.arange(n))
    ref = []
    for j in range(n):
        tcfg = dataclasses.replace(cfg, channel="table", table_h=h[j], reroll=False)
        ref.append(sim.run_trial(tcfg, dr["labels"][j], None, dr["z_noise"][j], dr["loc_u"][j], None, ITERS, True))
    ref = np.asarray(ref, np.int64)
    eng = rays_engine(cfg, prec)
    _, _, per = eng.run(seed, 0, n, ITERS, True, per_trial=True)
    eng.close()
    print("rays vs oracle", prec, per.sum(0), ref.sum(0))
    assert ref.sum() > 0
    if prec == "f64":
        assert_counts_equal(per, ref, "rays f64")
    else:
        assert_f32_counts_close(per, ref, "rays f32")


# ---------------------------------------------------------------- where the power goes
def test_one_specular_ray_points_signal_and_distortion():
    """An 8-element half-wavelength line array at 3.5 GHz, probes every 15 degrees on the circle of
    300 m at the array's height, soft limiter at IBO 1 dB, 64 trials.  A rays engine whose only ray is
    specular towards probe 4 (60 degrees) radiates its signal, its uncorrelated distortion and its
    out-of-band power towards that probe more than towards any other; a TDL engine with one tap
    (independent taps per antenna) has a flatter signal pattern.  The two engines are compared with
    each other: no directivity figure is fixed in advance."""
    cfg = dataclasses.replace(rays_cfg(8, 128, 256, M=16), ibo_db=1.0)
    k = 4
    probes = circle_probes(range(0, 181, 15), 300.0, cfg.array_z)
    f0 = rm.fftfreq_carriers(cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)[0]
    steer = scatterer_steering(cfg.tx_pos, probes[k:k + 1], f0)
    assert steer.shape == (8, 1)
    eng = engine_for(cfg, precision="f64")
    eng.set_rays([0], [0], [1.0], steer, [1])
    _, _, rows, _, _ = eng.beam(5, 0, 64, (0,), probes)
    eng.close()
    rays = _engine.BeamStats(rows, 64)
    eng = engine_for(cfg, precision="f64")
    eng.set_tdl([0], [1.0])
    _, _, rows, _, _ = eng.beam(5, 0, 64, (0,), probes)
    eng.close()
    tdl = _engine.BeamStats(rows, 64)
    for name in ("signal", "distortion", "power_oob"):
        v = getattr(rays, name)
        print(f"rays {name}: max/mean {v.max() / v.mean():.3f} at probe {int(np.argmax(v))}; "
              f"tdl max/mean {getattr(tdl, name).max() / getattr(tdl, name).mean():.3f}")
        assert int(np.argmax(v)) == k and np.all(np.delete(v, k) < v[k]), name
    assert tdl.directivity("signal") < rays.directivity("signal")
