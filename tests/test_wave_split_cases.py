"""CPU: pins the case table of tests/wave_split_cases.py, on the references alone.

The conditions are on the inputs of tests/test_gpu_wave_split_instances.py: a family that misses one
takes the next seed (wave_split_cases.SEEDS), the condition stays.  They are what lets the device
test compare exactly: counters neither empty nor saturated, trials that differ, no reliability or
sample within the allowed error of a bin edge.  Measured figures: profiles/r25/wave_split_matrix/README.md.
"""
import itertools
import os
import re

import numpy as np
import pytest

import ldpc_ref
import measure_ref
import wave_split_cases as ws
from test_gpu_soft import assert_reference_conditions

FAMILY_IDS = [fam.id for fam in ws.FAMILIES]
N_REL = {fam.id: fam.n_sc * int(np.log2(ws.CONSTEL)) for fam in ws.FAMILIES}


def test_the_table_is_the_full_cross_product():
    want = set(itertools.product(ws.SIZES, (True, False), ws.CHANNELS, (False, True)))
    keys = [fam.key for fam in ws.FAMILIES]
    assert len(keys) == 32 == len(set(keys)) and set(keys) == want
    assert len(set(FAMILY_IDS)) == 32 and len({fam.describe for fam in ws.FAMILIES}) == 32
    assert set(ws.SEEDS) <= want
    assert all(ws.BY_ID[i].key[1] is False for i in ws.MCNC_ROW_FAMILIES) and len(set(ws.MCNC_ROW_FAMILIES)) == 2
    assert all(fam.refused is None for fam in ws.FAMILIES)


def test_the_bands_are_what_the_slot_classes_need():
    """select_instance (engine.hip): aligned iff S % 4T == 0, S < F, S / T in (4, 8) and S / T < F / T."""
    for fam in ws.FAMILIES:
        t, s, f = ws.SIZES[fam.n_fft], fam.n_sc, fam.n_fft
        aligned = s % (4 * t) == 0 and s < f and s // t in (4, 8) and s // t < f // t
        assert aligned == fam.aligned, fam.id
        assert fam.slots == (4 if fam.aligned else 8)
        assert s % 4 == 0 and 4 <= s <= f - 2  # validate_config
        if not fam.aligned:
            assert s % 64 and s % t and s % (4 * t)
    assert ws.N_ANT > 1 and all(ws.N_ANT % (t // 64) for t in ws.SIZES.values())
    assert ws.BY_ID["F2048-generic-table-csi"].describe == "F=2048 T=256 slots=8 generic ch=4 csi=1 f64"
    assert ws.BY_ID["F1024-aligned-rayleigh"].describe == "F=1024 T=128 slots=4 aligned ch=1 csi=0 f64"


def test_mode_and_channel_numbers_are_the_headers():
    with open(os.path.join(ws.CSRC, "trial_params.h")) as f:
        modes = dict(re.findall(r"#define MIMO_MODE_(\w+) (\d)", f.read()))
    assert [int(modes[k]) for k in ("PLAIN", "MEAS", "SPEC", "BEAM", "ENV", "SOFT", "CODED")] == list(range(7))
    assert len(ws.MODES) == 7
    with open(os.path.join(ws.REPO, "include", "mimo_engine.h")) as f:
        chans = dict(re.findall(r"MIMO_CH_(\w+) = (\d)", f.read()))
    assert [int(chans[k]) for k in ("RAYLEIGH", "LOS", "TWOPATH", "TABLE")] == [ws.BY_ID[f"F1024-aligned-{c}"].ch
                                                                               for c in ws.CHANNELS]


def test_xaddr_masks_leave_out_25_of_112():
    masks = ws.left_out_masks()
    assert sorted(masks) == [1024, 2048]
    assert all(0 <= m <= 0xFF for ms in masks.values() for m in ms)
    assert sum(bin(m).count("1") for ms in masks.values() for m in ms) == 25
    grid = [(f, m, al, ch) for f in ws.SIZES for m in range(7) for al in (True, False) for ch in range(1, 5)]
    kept = [ws.holds_addresses(*g) for g in grid]
    assert (len(grid), sum(kept)) == (112, 87)
    # what tests/test_gpu_xaddr.py states: plain aligned Rayleigh re-derives at F 1024, LoS holds
    assert not ws.holds_addresses(1024, "plain", True, 1) and ws.holds_addresses(1024, "plain", True, 2)
    assert ws.holds_addresses(2048, 0, True, 1)  # the bench instance
    assert not ws.holds_addresses(2048, 0, True, 1, csi=True) and not ws.holds_addresses(512, 0, True, 1)
    # every mode has held instances; the modes with a mask of 0 have no other kind
    for f in ws.SIZES:
        for m in range(7):
            kinds = {ws.holds_addresses(f, m, al, ch) for al in (True, False) for ch in range(1, 5)}
            assert True in kinds and (False in kinds) == (masks[f][m] != 0)


@pytest.mark.parametrize("fid", FAMILY_IDS)
def test_counters_are_neither_empty_nor_saturated_and_trials_differ(fid):
    fam = ws.BY_ID[fid]
    ref = ws.reference(fam)
    assert ref.shape == (ws.TRIALS, 1 + len(ws.ITERS)) and np.all(ref >= 0)
    tot, bits = ref.sum(0), ws.TRIALS * N_REL[fid]
    print("WSPLIT_TOTALS", fid, "seed", fam.seed, tot.tolist(), "of", bits)
    assert np.all(tot >= 1), tot
    assert np.all(tot <= bits // 4), (tot, bits)
    assert len({tuple(r) for r in ref.tolist()}) > 1  # an all-equal answer proves nothing


@pytest.mark.parametrize("fid", FAMILY_IDS)
def test_row_references_count_what_the_oracle_counts(fid):
    fam = ws.BY_ID[fid]
    ref = ws.reference(fam)
    for mode in ("measure", "spectrum", "beam"):
        out = ws.reference(fam, mode)
        np.testing.assert_array_equal(out[0], ref, err_msg=mode)
        assert all(np.all(np.isfinite(a)) for a in out[1:])
    assert ws.reference(fam, "measure")[1].shape == (ws.TRIALS, measure_ref.MEAS_FIXED + 4)
    assert ws.reference(fam, "spectrum")[1].shape == (ws.TRIALS, fam.n_fft + 3)
    assert ws.reference(fam, "beam")[1].shape == (ws.TRIALS, ws.N_PROBES, 5)
    assert np.all(ws.reference(fam, "beam")[2] > 0)


def test_the_channels_of_a_class_can_be_told_apart():
    """An instance compiled with another family's Channel must not pass: within a (size, slot
    class, CSI) the channels' measure rows differ by more than 100 x the allowed deviation and their
    soft histograms differ.  (The counts alone do not tell LoS from two-path: the second path
    moves a handful of bits here.)"""
    for f, aligned, csi in itertools.product(ws.SIZES, (True, False), ws.CSI_EPS):
        fams = [ws.Family(f, aligned, ch, csi) for ch in ws.CHANNELS]
        for a, b in itertools.combinations(fams, 2):
            _, rows_a, ez_a = ws.reference(a, "measure")
            _, rows_b, _ = ws.reference(b, "measure")
            ratio = np.abs(rows_b - rows_a) / measure_ref.row_bounds(rows_a, ez_a)
            assert ratio[:, 4:].min() > 100.0, (a.id, b.id, float(ratio[:, 4:].min()))
            assert not np.array_equal(ws.reference(a, "soft")[1], ws.reference(b, "soft")[1]), (a.id, b.id)


@pytest.mark.parametrize("fid", FAMILY_IDS)
def test_soft_reference_is_exact(fid):
    """tests/test_gpu_soft.py assert_reference_conditions, for this family."""
    fam = ws.BY_ID[fid]
    counts, rows, near, nz = ws.reference(fam, "soft")
    print("WSPLIT_SOFT", fid, "near", near, "zeros", nz)
    np.testing.assert_array_equal(counts, ws.reference(fam))
    assert_reference_conditions(fid, fam.config(), counts, rows, near, nz)


@pytest.mark.parametrize("fid", FAMILY_IDS)
def test_coded_reference_is_exact(fid):
    fam = ws.BY_ID[fid]
    counts, chan, rows, dec_err, near, nz = ws.reference(fam, "coded")
    code = ws.ref_code()
    n_cw = N_REL[fid] // code.n_bits
    assert near == 0, f"{fid}: {near} reliabilities near a bin edge"
    assert nz == 0, f"{fid}: {nz} reliabilities are exactly 0"
    np.testing.assert_array_equal(counts, ws.reference(fam))
    assert chan.shape == (ws.TRIALS, 4, N_REL[fid]) and rows.shape == (ws.TRIALS, 4, 4) and n_cw >= 1
    assert np.all(chan % 2 != 0) and np.abs(chan).max() <= 63
    np.testing.assert_array_equal((chan < 0).sum(axis=2), counts)
    np.testing.assert_array_equal(rows[:, :, 0], dec_err)
    assert np.all(rows[:, :, 1] <= n_cw * code.n_bits) and np.all(rows[:, :, 2:] <= n_cw)
    assert np.all(rows[:, :, 3] <= rows[:, :, 2])


@pytest.mark.parametrize("fid", FAMILY_IDS)
def test_envelope_reference_is_exact(fid):
    fam = ws.BY_ID[fid]
    counts, rows, near = ws.reference(fam, "envelope")
    print("WSPLIT_ENVELOPE", fid, "near", near)
    assert near == 0, f"{fid}: {near} samples near a bin edge"
    np.testing.assert_array_equal(counts, ws.reference(fam))
    nb, n_samp = 128, ws.N_ANT * fam.n_fft
    assert rows.shape == (ws.TRIALS, 260)
    assert np.all(rows[:, :nb].sum(1) == n_samp) and np.all(rows[:, nb:2 * nb].sum(1) == n_samp)


def test_the_families_hold_corrected_and_failed_frames():
    """tests/test_gpu_ldpc_seam.py's rule, over all families: in the reference at least one frame
    fails and at least one frame with channel errors is corrected."""
    code = ws.ref_code()
    failed = corrected = 0
    for fam in ws.FAMILIES:
        _, chan, rows, _, _, _ = ws.reference(fam, "coded")
        failed += int(rows[:, :, 2].sum())
        raw = (ldpc_ref.codewords(code, chan) < 0).any(axis=-1).sum()     # frames with channel errors
        corrected += int(raw - rows[:, :, 2].sum())
    print("WSPLIT_FRAMES failed", failed, "with channel errors and decoded", corrected)
    assert failed >= 1 and corrected >= 1, (failed, corrected)


def test_references_are_cached_and_read_only():
    fam = ws.FAMILIES[0]
    assert ws.reference(fam) is ws.reference(fam, "plain", "cnc")
    with pytest.raises(ValueError):
        ws.reference(fam)[0, 0] = 1
    with pytest.raises(ValueError):
        ws.reference(fam, "soft")[1][0, 0, 0] = 1
