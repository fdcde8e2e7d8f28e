"""The channel bank of the table engines (mimo_engine_set_channel_bank) on the GPU: trial i reads
table i mod n_bank.  Pinned by the reference's own per-trial counts (the golden fixtures' channels
as one bank), and against single-table engines run one trial at a time -- the same device code on
the same H, so every comparison is exact -- over both geometries' slot maps, both receivers, both
precisions, split calls, multi-point launches, every row mode and sequences of banks.
"""
import dataclasses
import functools

import numpy as np
import pytest

from conftest import link_fixture_names, load_golden, sim_config_from_fixture
from gpu_util import PRECISIONS, assert_counts_equal, engine_for
from oracle import sim
from test_gpu_beam import probes_n
from utilities import qc_ldpc_code

pytestmark = pytest.mark.gpu

SEED = 23
ITERS = (0, 1, 2)
GEOMETRIES = [(8, 256, 512), (3, 100, 128)]  # aligned slots; generic slots, a band that is no multiple of a wave


@functools.lru_cache(maxsize=None)
def tables(n, A, F):
    rng = np.random.default_rng(1000 * n + 10 * A + F)
    h = (rng.standard_normal((n, A, F)) + 1j * rng.standard_normal((n, A, F))) * np.sqrt(0.5) * 3e-7
    h.setflags(write=False)
    return h


def table_cfg(A, S, F, receiver="cnc", M=16, **kw):
    return sim.SimConfig(A, S, F, M, ibo_db=1.0, snr_db=14.0, channel="table", receiver=receiver, reroll=False, **kw)


def bank_engine(cfg, bank, prec):
    eng = engine_for(dataclasses.replace(cfg, table_h=bank[0]), precision=prec)
    eng.set_channel_bank(bank)
    return eng


def single_trials(cfg, bank, prec, seed, trials, fn=None):
    """Trial t on a single-table engine holding table t mod n_bank, one trial per call.
    fn(engine, seed, t) makes the call (default: the plain run's per-trial counts)."""
    fn = fn or (lambda eng, seed, t: eng.run(seed, t, 1, ITERS, True, per_trial=True)[2])
    engines = [engine_for(dataclasses.replace(cfg, table_h=h), precision=prec) for h in bank]
    out = [fn(engines[t % len(bank)], seed, t) for t in trials]
    for e in engines:
        e.close()
    return out


# ---------------------------------------------------------------- the reference's own counts
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", [n for n in link_fixture_names() if n != "csi_cnc"])
def test_bank_vs_reference_fixture(name, prec):
    """The channels H_j of a golden fixture's first trials as one bank: one run over trials 0 .. n - 1
    gives the reference's counts of those trials exactly (what
    test_gpu_engine.py::test_table_channel_vs_reference_fixture gets from n engines, a trial each)."""
    g = load_golden(f"link_{name}.npz")
    cfg = sim_config_from_fixture(g)
    n = min(int(g["n_trials"]), 6)
    d = sim.draws(cfg, int(g["seed"]), np.arange(n))
    bins = sim.rm.inband_bins(cfg.n_fft, cfg.n_sc)
    bank = np.zeros((n, cfg.n_ant, cfg.n_fft), complex)
    for j in range(n):
        bank[j][:, bins] = sim.channel_inband(cfg, d["z_chan"][j], d["loc_u"][j])
    eng = bank_engine(dataclasses.replace(cfg, channel="table", reroll=False), bank, prec)
    assert "ch=4" in eng.describe()
    err, _, per = eng.run(int(g["seed"]), 0, n, g["iters"], bool(g["incl_clean"]), per_trial=True)
    print(name, prec, eng.describe(), per.sum(0), g["counts"][:n].sum(0))
    eng.close()
    assert_counts_equal(per, g["counts"][:n], f"{name} bank {prec}")
    np.testing.assert_array_equal(err, per.sum(0))


# ---------------------------------------------------------------- indexing
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("receiver", ["cnc", "mcnc"])
@pytest.mark.parametrize("A,S,F", GEOMETRIES)
def test_trial_reads_table_trial_mod_n_bank(A, S, F, receiver, prec):
    cfg = table_cfg(A, S, F, receiver)
    bank = tables(3, A, F)
    eng = bank_engine(cfg, bank, prec)
    _, _, per = eng.run(SEED, 5, 7, ITERS, True, per_trial=True)
    want = np.concatenate(single_trials(cfg, bank, prec, SEED, range(5, 12)))
    np.testing.assert_array_equal(per, want)
    assert len({tuple(r) for r in per.tolist()}) > 1  # the trials differ: an all-equal answer proves nothing
    # the same call split at trial 8
    _, _, a = eng.run(SEED, 5, 3, ITERS, True, per_trial=True)
    _, _, b = eng.run(SEED, 8, 4, ITERS, True, per_trial=True)
    np.testing.assert_array_equal(np.concatenate([a, b]), per)
    # two points with different seeds, first trials and IBO in one launch
    other = engine_for(dataclasses.replace(cfg, ibo_db=3.0, table_h=bank[0]), precision=prec)
    points, seeds, first, n = [eng.point_kw, other.point_kw], [SEED, SEED + 1], [5, 1], [4, 6]
    other.close()
    _, _, both = eng.run_points(points, seeds, first, n, ITERS, True, per_trial=True)
    sep = [eng.run_points([points[i]], [seeds[i]], [first[i]], [n[i]], ITERS, True, per_trial=True)[2] for i in (0, 1)]
    np.testing.assert_array_equal(both, np.concatenate(sep))
    np.testing.assert_array_equal(sep[0], per[:4])
    want1 = np.concatenate(single_trials(dataclasses.replace(cfg, ibo_db=3.0), bank, prec, SEED + 1, range(1, 7)))
    np.testing.assert_array_equal(sep[1], want1)
    eng.close()


# ---------------------------------------------------------------- every row mode
ROW_CFG = table_cfg(4, 100, 256, M=64)
CODE = qc_ldpc_code(16, 3, 6)


def mode_call(mode, eng, seed, first, n):
    """-> the per-trial arrays of the call (counts first)."""
    if mode == "plain":
        return [eng.run(seed, first, n, ITERS, True, per_trial=True)[2]]
    if mode == "measure":
        out = eng.measure(seed, first, n, ITERS, True, per_trial=True)
    elif mode == "spectrum":
        out = eng.spectrum(seed, first, n, ITERS, True, per_trial=True)
    elif mode == "beam":
        out = eng.beam(seed, first, n, ITERS, probes_n(5), True, per_trial=True)
    elif mode == "envelope":
        out = eng.envelope(seed, first, n, ITERS, 1e-13, True, per_trial=True)
    elif mode == "soft":
        out = eng.soft(seed, first, n, ITERS, 8.0, True, per_trial=True)
    else:
        out = eng.coded(seed, first, n, ITERS, CODE, 8.0, True, True, chan=True)
    return list(out[3:])


@pytest.mark.parametrize("mode", ["plain", "measure", "spectrum", "beam", "envelope", "soft", "coded"])
def test_every_row_mode_reads_the_bank(mode):
    bank = tables(2, 4, 256)
    eng = bank_engine(ROW_CFG, bank, "f64")
    got = mode_call(mode, eng, SEED, 0, 4)
    eng.close()
    want = single_trials(ROW_CFG, bank, "f64", SEED, range(4), lambda e, seed, t: mode_call(mode, e, seed, t, 1))
    assert len(got) == len(want[0]) >= 1
    for k, g in enumerate(got):
        w = np.concatenate([row[k] for row in want])
        assert g.shape == w.shape and g.shape[0] == 4
        np.testing.assert_array_equal(g, w, err_msg=f"{mode} output {k}")
        if k > 0:
            assert np.any(g[0] != g[1])  # rows of trials on different tables differ


# ---------------------------------------------------------------- sequences of banks
@pytest.mark.parametrize("prec", PRECISIONS)
def test_bank_sequence_equals_fresh_engines(prec):
    """A bank of 4, then one of 2, then n_bank = 0: each call returns the bits of a fresh engine in
    that state (the device copy is replaced, larger or smaller, at the next run)."""
    cfg = table_cfg(3, 100, 128)
    big, small = tables(4, 3, 128), tables(2, 3, 128)
    eng = engine_for(dataclasses.replace(cfg, table_h=big[0]), precision=prec)

    def run(e):
        return e.run(SEED, 2, 9, ITERS, True, per_trial=True)

    def fresh(bank):
        e = engine_for(dataclasses.replace(cfg, table_h=big[0]), precision=prec)
        if bank is not None:
            e.set_channel_bank(bank)
        out = run(e)
        e.close()
        return out

    base = run(eng)  # the create-time table, before any bank
    seen = []
    for bank in (big, small, None, small[:1], big):
        eng.set_channel_bank(bank)
        got, want = run(eng), fresh(bank)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        seen.append(got[2])
    np.testing.assert_array_equal(seen[2], base[2])       # n_bank = 0: the create-time table again
    np.testing.assert_array_equal(seen[0], seen[4])
    assert np.any(seen[0] != seen[1]) and np.any(seen[1] != seen[2]) and np.any(seen[3] != seen[2])
    eng.close()


def test_bank_and_beam_calls_in_either_order():
    bank = tables(2, 4, 256)

    def calls(order):
        eng = bank_engine(ROW_CFG, bank, "f64")
        out = {m: mode_call(m, eng, SEED, 1, 5) for m in order}
        eng.close()
        return out

    a, b = calls(["beam", "plain", "soft"]), calls(["soft", "plain", "beam"])
    for m in a:
        for g, w in zip(a[m], b[m]):
            np.testing.assert_array_equal(g, w, err_msg=m)
    np.testing.assert_array_equal(a["plain"][0], a["beam"][0])  # and the modes agree on the counts
