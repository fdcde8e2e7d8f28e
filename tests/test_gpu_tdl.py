"""The tapped-delay-line channel on the GPU: the fine seam mimo_tdl_channels against the long-double
reference (tests/tdl_ref.py), the engine's generator against the seam (a bank engine holding the
seam's matrices must give the same bits), the split of long calls at the bank's capacity, and a TDL
engine's per-trial counts against the oracle run on the seam's channels.
"""
import dataclasses

import numpy as np
import pytest

import _engine
import tdl_ref
from gpu_util import PRECISIONS, assert_counts_equal, assert_f32_counts_close, engine_for
from oracle import sim
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu

FACTOR = 16.0  # tests/test_gpu_stage_kernels.py test_awgn_values' yardstick factor
HIGH_SEED = 0xFEDCBA9876543210
ITERS = (0, 1, 2)


def spread_delays(n_taps, n_fft):
    """n_taps ascending delays from 0 up to n_fft - 1, unevenly spaced."""
    inner = np.random.default_rng(n_fft).choice(np.arange(1, n_fft - 1), n_taps - 2, replace=False)
    return np.sort(np.concatenate(([0], inner, [n_fft - 1])))


def profile(kind, n_fft):
    if kind == "one@0":
        return np.array([0]), np.array([1.7])
    if kind == "one@5":
        return np.array([5]), np.array([0.6])
    d = spread_delays(64, n_fft)
    return d, 10 ** (-np.arange(64) / 20.0)


# (profile, n_fft, n_ant, n, first_trial, seed): every listed value of each appears, the extremes together
SEAM_CASES = [("one@0", 128, 1, 1, 0, 1), ("one@0", 8192, 3, 5, 7, HIGH_SEED), ("one@5", 128, 3, 5, 2 ** 32 - 2, 77),
              ("one@5", 8192, 1, 1, 3, HIGH_SEED), ("L64", 128, 3, 1, 2 ** 32 - 2, HIGH_SEED), ("L64", 8192, 3, 5, 11, 5),
              ("L64", 128, 1, 5, 0, 9)]


@pytest.mark.parametrize("kind,F,A,n,first,seed", SEAM_CASES, ids=[f"{c[0]}-F{c[1]}-A{c[2]}-n{c[3]}" for c in SEAM_CASES])
def test_seam_accuracy(kind, F, A, n, first, seed):
    delays, powers = profile(kind, F)
    L = len(delays)
    amp = None if A == 1 else np.linspace(0.5, 1.25, A)
    h, g = _engine.tdl_channels(delays, powers, A, F, seed, first, n, ant_amp=amp, taps=True)
    assert h.shape == (n, A, F) and g.shape == (n, A, L)
    # taps: error relative to |g| against 16 times NumPy's own on the same elements (on at least 257:
    # a few samples' may be small by luck, as test_awgn_values widens its n = 1 case)
    n_y = max(n, -(-257 // (A * L)))
    ty = [first + j for j in range(n_y)]
    ld = tdl_ref.ld_taps(powers, A, seed, ty, amp)
    e_np = float(np.max(np.abs(tdl_ref.np_taps(powers, A, seed, ty, amp) - ld) / np.abs(ld)))
    err = float(np.max(np.abs(g - ld[:n]) / np.abs(ld[:n])))
    print(f"taps: device {err:.3e}, NumPy {e_np:.3e} (bound {FACTOR * e_np:.3e})")
    assert e_np > 0 and err <= FACTOR * e_np
    # transform: H against the long-double DFT of the device's own taps
    ref = tdl_ref.ld_response(g, delays, F)
    bound = (L + 8) * 2.0 ** -53 * np.sum(np.abs(g), axis=-1, keepdims=True)
    dev = h - ref
    worst = float(np.max(np.maximum(np.abs(dev.real), np.abs(dev.imag)) / bound))
    print(f"transform: worst error / bound {worst:.3f}")
    assert np.all(np.abs(dev.real) <= bound) and np.all(np.abs(dev.imag) <= bound)
    assert np.all(np.isfinite(h.view(np.float64)))
    if kind == "one@0":  # W[0] = 1 exactly: flat at the tap, bit for bit
        assert np.array_equal(h, np.broadcast_to(g, h.shape))
    # trial indices are taken mod 2^32
    if first + n > 2 ** 32:
        k = 2 ** 32 - first
        np.testing.assert_array_equal(h[k:], _engine.tdl_channels(delays, powers, A, F, seed, 0, n - k, ant_amp=amp))


def test_seam_streams_are_distinct_and_repeatable():
    d, p = [0, 3], [1.0, 1.0]
    base = _engine.tdl_channels(d, p, 2, 128, 0x1234, 4, 2, taps=True)[1]
    vals = [base[0, 0, 0], base[0, 1, 0], base[0, 0, 1], base[1, 0, 0]]  # then: antenna, tap, trial changed
    vals.append(_engine.tdl_channels(d, p, 2, 128, 0x1235, 4, 2, taps=True)[1][0, 0, 0])             # seed, low word
    vals.append(_engine.tdl_channels(d, p, 2, 128, 0x1234 | (1 << 40), 4, 2, taps=True)[1][0, 0, 0])  # seed, high word
    assert len(set(vals)) == len(vals) and len({v.real for v in vals}) == len(vals)
    again = _engine.tdl_channels(d, p, 2, 128, 0x1234, 4, 2, taps=True)[1]
    np.testing.assert_array_equal(again, base)
    np.testing.assert_array_equal(_engine.tdl_channels(d, p, 2, 128, 0x1234, 5, 1, taps=True)[1][0], base[1])


# ---------------------------------------------------------------- the engine's generator
def tdl_cfg(A, S, F, receiver="cnc", M=16):
    return sim.SimConfig(A, S, F, M, ibo_db=1.0, snr_db=14.0, channel="tdl", receiver=receiver)


def tdl_profile_for(A, F):
    return np.array([0, 2, 5, F // 4 + 1]), np.array([0.5, 0.25, 0.15, 0.1]), np.linspace(0.5, 1.0, A)


def tdl_engine(cfg, prec):
    eng = engine_for(cfg, precision=prec)
    eng.set_tdl(*tdl_profile_for(cfg.n_ant, cfg.n_fft))
    assert "ch=4" in eng.describe()  # the table instances
    return eng


def bank_of_seam(cfg, prec, seed, t0, n):
    """A bank engine holding the seam's matrices of trials t0 .. t0 + n - 1, ordered by trial mod n."""
    d, p, amp = tdl_profile_for(cfg.n_ant, cfg.n_fft)
    h = _engine.tdl_channels(d, p, cfg.n_ant, cfg.n_fft, seed, t0, n, ant_amp=amp)
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
    cfg = tdl_cfg(A, S, F, receiver)
    eng = tdl_engine(cfg, prec)
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


@pytest.mark.parametrize("mode", ["soft", "coded"])
def test_engine_generator_equals_the_seam_in_row_modes(mode):
    cfg = tdl_cfg(4, 100, 256, M=64)
    code = qc_ldpc_code(16, 3, 6)

    def call(e):
        if mode == "soft":
            return e.soft(31, 7, 5, ITERS, 8.0, True, per_trial=True)
        return e.coded(31, 7, 5, ITERS, code, 8.0, True, True, chan=True)

    eng, ref = tdl_engine(cfg, "f64"), bank_of_seam(cfg, "f64", 31, 7, 5)
    got, want = call(eng), call(ref)
    eng.close()
    ref.close()
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{mode} output {k}")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_long_calls_split_at_the_bank_capacity(prec):
    """Config-2 geometry: one call of capacity + 3 trials runs as two launches, and its per-trial
    counts equal those of the same trials run as two calls split elsewhere."""
    cfg = dataclasses.replace(tdl_cfg(64, 1024, 2048, M=64), ibo_db=3.0, snr_db=25.0)
    cap = _engine.bank_capacity(64, 1024, prec)
    assert cap == (1024 if prec == "f64" else 2048)
    eng = tdl_engine(cfg, prec)
    n = cap + 3
    err, bits, per = eng.run(5, 0, n, [0], False, per_trial=True)
    _, _, a = eng.run(5, 0, 1000, [0], False, per_trial=True)
    _, _, b = eng.run(5, 1000, n - 1000, [0], False, per_trial=True)
    eng.close()
    np.testing.assert_array_equal(per, np.concatenate([a, b]))
    np.testing.assert_array_equal(err, per.sum(0))
    assert int(bits[0]) == n * 1024 * 6 and len(np.unique(per)) > 1


# ---------------------------------------------------------------- the oracle on the seam's channels
@pytest.mark.parametrize("prec", PRECISIONS)
def test_tdl_engine_vs_oracle(prec):
    """A 8, S 256, F 512, L 4, CNC iterations 0, 1 and 2, 16 trials: oracle.sim.run_trial with
    channel="table" and table_h the seam's H of the trial, labels and noise from sim.draws.
    float64: exact; float32: the project's float32 criterion (gpu_util.assert_f32_counts_close)."""
    cfg = tdl_cfg(8, 256, 512)
    seed, n = 2137, 16
    d, p, amp = tdl_profile_for(8, 512)
    h = _engine.tdl_channels(d, p, 8, 512, seed, 0, n, ant_amp=amp)
    dr = sim.draws(cfg, seed, np.arange(n))
    ref = []
    for j in range(n):
        tcfg = dataclasses.replace(cfg, channel="table", table_h=h[j], reroll=False)
        ref.append(sim.run_trial(tcfg, dr["labels"][j], None, dr["z_noise"][j], dr["loc_u"][j], None, ITERS, True))
    ref = np.asarray(ref, np.int64)
    eng = tdl_engine(cfg, prec)
    _, _, per = eng.run(seed, 0, n, ITERS, True, per_trial=True)
    eng.close()
    print("tdl vs oracle", prec, per.sum(0), ref.sum(0))
    assert ref.sum() > 0
    if prec == "f64":
        assert_counts_equal(per, ref, "tdl f64")
    else:
        assert_f32_counts_close(per, ref, "tdl f32")
