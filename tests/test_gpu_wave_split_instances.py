"""Every float64 wave-split instance (F 1024, F 2048; csrc/wave_fft.h) in all seven run modes on the
GPU: tests/wave_split_cases.py's 32 families -- size x slot class x channel x CSI -- each through
plain, measure, spectrum, beam, envelope, soft and coded on one engine, 224 kernels, those that hold
their transform addresses across the antenna loop and those that re-derive them (csrc/trial_kernel.h
xaddr_inst_ok) alike.

Per family ``describe()`` must be the family's text, or the test is not running the instance it
claims.  Counts are the oracle's per trial, exactly, in every mode, and the plain run's; rows are held
to the bound of the mode's own test, imported from it: measure_ref.row_bounds,
spectrum_ref.row_bounds, beam_ref's bounds, test_gpu_envelope.check_rows, and cell for cell for the
soft histograms, the coded rows and the channel values.  The exact comparisons stand on the
conditions tests/test_wave_split_cases.py pins on the references.  Every output is finite and a
second identical call returns the same bits.  Plain mode runs again under MCNC, and two generic
families (wave_split_cases.MCNC_ROW_FAMILIES) run the six row modes under MCNC too: the held words
live through the MCNC passes.  A mode's failure is collected and asserted at the end, so it does
not hide another mode's.

One line per (family, mode):
    WSPLIT|<describe>|<mode>|held=<0|1>|gpu=<column sums>|oracle=<column sums>|<worst ratio to the bound>
The lines of a passing run: profiles/r25/wave_split_matrix/README.md.
"""
import functools

import numpy as np
import pytest

import _engine
import measure_ref
import spectrum_ref
import wave_split_cases as ws
from gpu_util import assert_counts_equal, engine_for
from test_gpu_beam import assert_totals, probes_n
from test_gpu_envelope import NB, check_rows

pytestmark = pytest.mark.gpu

N = ws.TRIALS
ITERS = ws.ITERS


@functools.lru_cache(maxsize=None)
def device_code():
    code = ws.ref_code()
    return _engine.LdpcCode(code.z, code.shifts, code.n_dec_iters)


def call(eng, fam, mode):
    """The mode's call on trials 0-3 -> (err, bits, per-trial counts, [totals, per-trial rows, ...])."""
    seed = fam.seed
    if mode == "plain":
        err, bits, per = eng.run(seed, 0, N, ITERS, True, per_trial=True)
        return err, bits, per, []
    if mode == "measure":
        out = eng.measure(seed, 0, N, ITERS, True, per_trial=True)
    elif mode == "spectrum":
        out = eng.spectrum(seed, 0, N, ITERS, True, per_trial=True)
    elif mode == "beam":
        out = eng.beam(seed, 0, N, ITERS, probes_n(ws.N_PROBES), True, per_trial=True)
    elif mode == "envelope":
        out = eng.envelope(seed, 0, N, ITERS, ws.ref_pow(fam), True, per_trial=True)
    elif mode == "soft":
        out = eng.soft(seed, 0, N, ITERS, ws.RHO_MAX, True, per_trial=True)
    else:
        out = eng.coded(seed, 0, N, ITERS, device_code(), ws.RHO_MAX, True, per_trial=True, chan=True)
    return out[0], out[1], out[3], [out[2]] + list(out[4:])


def check_mode(eng, fam, mode, receiver, plain):
    """One mode of one family: its counts, rows and repeatability; -> its WSPLIT line's tail."""
    ref = ws.reference(fam, mode, receiver)
    ref_counts = ref if mode == "plain" else ref[0]
    err, bits, per, rows = call(eng, fam, mode)
    label = f"{fam.id} {mode} {receiver}"
    worst = ""
    try:
        assert_counts_equal(per, ref_counts, f"{label}: vs oracle")
        np.testing.assert_array_equal(err, per.sum(0), err_msg=f"{label}: totals")
        assert np.all(bits == N * fam.n_sc * 4)
        if plain is not None:
            assert_counts_equal(per, plain, f"{label}: vs the plain run")
        assert all(np.all(np.isfinite(a)) for a in rows), f"{label}: not finite"
        if mode == "measure":
            tot, pr = rows
            assert pr.shape == ref[1].shape
            ratio = float((np.abs(pr - ref[1]) / measure_ref.row_bounds(ref[1], ref[2])).max())
            worst = f"{ratio:.3e}"
            assert ratio <= 1.0, f"{label}: a row deviates {ratio:.3g} x its bound"
            np.testing.assert_allclose(tot, pr.sum(0), rtol=1e-12, atol=0)
        elif mode == "spectrum":
            tot, pr = rows
            assert pr.shape == ref[1].shape
            ratio = float((np.abs(pr - ref[1]) / spectrum_ref.row_bounds(ref[1])).max())
            worst = f"{ratio:.3e}"
            assert ratio <= 1.0, f"{label}: a row deviates {ratio:.3g} x its bound"
            np.testing.assert_allclose(tot, pr.sum(0), rtol=1e-12, atol=0)
        elif mode == "beam":
            tot, pr = rows
            assert pr.shape == ref[1].shape
            ratio = float((np.abs(pr - ref[1]) / ref[2]).max())
            worst = f"{ratio:.3e}"
            assert ratio <= 1.0, f"{label}: a row deviates {ratio:.3g} x its bound"
            assert_totals(tot, pr)
        elif mode == "envelope":
            tot, pr = rows
            assert ref[2] == 0
            fixed = np.abs(pr[:, 2 * NB:] - ref[1][:, 2 * NB:]) / (1e-12 * ref[1][:, 2 * NB:2 * NB + 1])
            worst = f"{float(fixed.max()):.3e}"
            check_rows(label, pr, ref[1])
            np.testing.assert_array_equal(tot[:2 * NB], pr[:, :2 * NB].sum(0))
            np.testing.assert_allclose(tot[2 * NB:], pr[:, 2 * NB:].sum(0), rtol=1e-12, atol=1e-12 * tot[2 * NB])
        elif mode == "soft":
            tot, pr = rows
            assert ref[2] == 0 and ref[3] == 0
            np.testing.assert_array_equal(pr, ref[1], err_msg=f"{label}: per-trial rows")
            np.testing.assert_array_equal(tot, pr.sum(axis=0))
        elif mode == "coded":
            tot, pr, chan = rows
            assert ref[4] == 0 and ref[5] == 0
            assert chan.dtype == np.int8 and chan.shape == ref[1].shape
            np.testing.assert_array_equal(chan, ref[1], err_msg=f"{label}: channel values")
            np.testing.assert_array_equal(pr, ref[2], err_msg=f"{label}: per-trial rows")
            np.testing.assert_array_equal(tot, pr.sum(axis=0))
        # a second identical call: the same bits
        err2, bits2, per2, rows2 = call(eng, fam, mode)
        np.testing.assert_array_equal(per2, per, err_msg=f"{label}: second call, counts")
        np.testing.assert_array_equal(err2, err)
        for a, b in zip(rows, rows2):
            assert np.array_equal(a, b), f"{label}: second call differs in {int((a != b).sum())} cells"
        failure = None
    except AssertionError as e:
        failure = f"{label}: {e}"
    tag = mode if receiver == "cnc" else f"{mode}/{receiver}"
    print(f"WSPLIT|{eng.describe()}|{tag}|held={int(ws.held(fam, mode))}|gpu={per.sum(0).tolist()}"
          f"|oracle={ref_counts.sum(0).tolist()}|{worst}")
    return per, failure


@pytest.mark.parametrize("fid", [fam.id for fam in ws.FAMILIES])
def test_family_in_every_mode(fid):
    fam = ws.BY_ID[fid]
    if fam.refused is not None:
        with pytest.raises(ValueError, match=fam.refused):
            engine_for(fam.config(), precision="f64")
        return
    failures = []
    print()  # the WSPLIT lines start their own lines under -v -s
    for receiver in ("cnc", "mcnc"):
        eng = engine_for(fam.config(receiver), precision="f64")
        assert eng.describe() == fam.describe, (eng.describe(), fam.describe)
        modes = ws.MODES if receiver == "cnc" or fid in ws.MCNC_ROW_FAMILIES else ws.MODES[:1]
        plain = None
        for mode in modes:
            per, failure = check_mode(eng, fam, mode, receiver, plain)
            if mode == "plain":
                plain = per
            if failure:
                failures.append(failure)
        assert eng.describe() == fam.describe
        eng.close()
    assert not failures, f"{len(failures)} of the modes failed:\n" + "\n".join(failures)
