"""Values, not decisions: every production FFT instance of the trial kernel (team, wave-split,
split; float64 and float32, both exchange-buffer counts and both float32 team sizes), run
through libmimo_probe as the kernel runs it -- IFFT -> PA -> FFT on the instance's registers,
tables and LDS helpers -- against the same chain in long double (tests/probe_util.py).

Bound: NumPy's own chain in the instance's precision (np.fft keeps complex64 / complex128) has
an error e_np against the long-double reference at the same input (the worst of the input's
three rows); each row of the device's result may lose a factor 16 (4 bits) against it, in the
relative l2 norm and in the largest deviation over rms(ref).
pocketfft is close to the best attainable, a radix-8/16 Stockham that forms some twiddles as
products of table entries can lose a small factor -- a float-rounded table or a dropped Newton
step in a float64 instance loses six orders of magnitude (the CPU self-checks below, and
tests/test_probe_tables.py on the production cot-tan constants).

Measured on an MI355X (profiles/r07/probe/accuracy.md): every instance stays within 3.1 x
e_np in l2 and 4.9 x in the largest deviation (float64 l2 1.0e-16 .. 3.6e-16, float32 0.9e-7 ..
2.3e-7)."""
import functools

import numpy as np
import pytest

import probe_util as pu

gpu = pytest.mark.gpu
FACTOR = 16.0
ROWS = 3
# (name, PA kind, Rapp hardness); saturation = mean sample power, third-order c = 0.05 / mean power
MODES = [("identity", pu.PA_NONE, 0.0), ("softlim", pu.PA_SOFTLIM, 0.0), ("rapp3", pu.PA_RAPP, 3.0),
         ("rapp2.5", pu.PA_RAPP, 2.5), ("toi", pu.PA_TOI, 0.0)]
INPUTS = ["qam", "normal", "onehot"]


def band_bins(F):
    """The engine's bin map of S = F / 2 sub-carriers (modulation.py:266-267)."""
    S = F // 2
    return np.concatenate([np.arange(F - S // 2, F), np.arange(1, S // 2 + 1)])


@functools.lru_cache(maxsize=None)
def make_input(prec, F, kind):
    """[ROWS][F] in the instance's complex type, and whether the masked variant runs."""
    rng = np.random.default_rng(1000 * F + 10 * INPUTS.index(kind) + prec)
    X = np.zeros((ROWS, F), np.complex128)
    if kind == "qam":  # in-band 64-QAM lattice points / sqrt(F)
        b = band_bins(F)
        lv = np.arange(-7, 8, 2)
        X[:, b] = (rng.choice(lv, (ROWS, b.size)) + 1j * rng.choice(lv, (ROWS, b.size))) / np.sqrt(F)
    elif kind == "normal":  # full band
        X[:] = (rng.standard_normal((ROWS, F)) + 1j * rng.standard_normal((ROWS, F))) * np.sqrt(0.5)
    else:  # one bin per row: the first, the quarter turn (the table's tan is 4e19 there) and the band's lower edge
        for r, b in enumerate((1, F // 4, F - F // 4)):
            X[r, b] = 0.75 - 1.25j
    X = X.astype(pu.cdtype(prec))  # the reference starts from the rounded values
    X.setflags(write=False)
    return X, kind == "qam"


@functools.lru_cache(maxsize=None)
def pa_params(prec, F, kind):
    """(sat, toi coefficient), rounded to the instance's type (what the device is handed)."""
    X, _ = make_input(prec, F, kind)
    x = pu.ld_fft(X, +1)
    mean_pw = float(np.mean(np.abs(x) ** 2))
    rt = pu.rdtype(prec)
    return float(rt(mean_pw)), float(rt(0.05 / mean_pw))


@functools.lru_cache(maxsize=None)
def reference(prec, F, kind, mode):
    """The long-double chain and NumPy's errors (l2, max-abs per row) against it.  Shared by
    every variant of (prec, F); never modified."""
    X, _ = make_input(prec, F, kind)
    sat, toi = pa_params(prec, F, kind)
    _, pk, p = MODES[[m[0] for m in MODES].index(mode)]
    ref = pu.ld_chain(X, pk, sat, p, toi)
    ref.setflags(write=False)
    # NumPy's error at this input: the worst of its rows.  (Row by row it can be exactly 0 -- a
    # single bin at the quarter turn meets only twiddles +-1 and +-j -- which bounds nothing.)
    e_np = tuple(np.full(ROWS, e.max()) for e in pu.errors(pu.np_chain(np.array(X), pk, sat, p, toi), ref))
    assert e_np[0][0] > 0 and e_np[1][0] > 0
    return ref, e_np


def within(got, ref, e_np):
    """Per row: both metrics within FACTOR x NumPy's.  Returns (ok, l2, mx)."""
    l2, mx = pu.errors(got, ref)
    ok = np.all(l2 <= FACTOR * e_np[0]) and np.all(mx <= FACTOR * e_np[1])
    return bool(ok), l2, mx


# ---------------------------------------------------------------- CPU self-checks
def test_long_double_fft_equals_the_direct_dft():
    rng = np.random.default_rng(3)
    for n in (2, 8, 64, 256):
        x = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))).astype(pu.CLD)
        for sign in (-1, +1):
            l2, mx = pu.errors(pu.ld_fft(x, sign), pu.ld_dft_direct(x, sign))
            assert np.all(l2 < 1e-18) and np.all(mx < 1e-17), (n, sign, l2, mx)
    # and against NumPy at float64 level, with the sign convention of np.fft
    x = rng.standard_normal(512) + 1j * rng.standard_normal(512)
    l2, _ = pu.errors(np.fft.fft(x)[None], pu.ld_fft(x[None], -1))
    assert l2[0] < 1e-15
    l2, _ = pu.errors(np.fft.ifft(x)[None] * 512, pu.ld_fft(x[None], +1))
    assert l2[0] < 1e-15


@pytest.mark.parametrize("F", [128, 2048, 8192])
@pytest.mark.parametrize("mode", ["identity", "rapp2.5"])
def test_metric_rejects_single_precision_and_one_perturbed_bin(F, mode):
    """The float64 bound has teeth: a float32-rounded copy of the reference, and the reference
    with one bin off by 1e-12 relative, both fall outside 16 x e_np."""
    ref, e_np = reference(0, F, "normal", mode)
    assert np.all(e_np[0] > 5e-17) and np.all(e_np[0] < 2e-15), e_np  # NumPy itself: float64 level
    ok, l2, mx = within(np.array(ref).astype(np.complex64), ref, e_np)
    assert not ok and np.all(l2 > 1e5 * FACTOR * e_np[0])
    bad = np.array(ref)
    k = int(np.argmax(np.abs(bad[0])))
    bad[0, k] *= pu.LD(1) + pu.LD(1e-12)
    ok, l2, mx = within(bad, ref, e_np)
    assert not ok
    assert l2[0] > FACTOR * e_np[0][0] and mx[0] > FACTOR * e_np[1][0], (l2[0], mx[0], e_np)
    ok, _, _ = within(np.array(ref), ref, e_np)
    assert ok


# ---------------------------------------------------------------- the device
def _id(inst):
    prec, F, v = inst
    return f"{'f64' if prec == 0 else 'f32'}-F{F}-v{v}"


@gpu
@pytest.mark.parametrize("inst", pu.fft_instances(), ids=_id)
def test_fft_pa_fft_chain_against_long_double(inst):
    prec, F, variant = inst
    T, zm, fft_kind = pu.fft_info(prec, F, variant)
    failures = []
    for kind in INPUTS:
        X, masked = make_input(prec, F, kind)
        if masked:  # the production mask clears out-of-band bins only: the reference input has them zero
            assert not np.any(np.array(X)[:, pu.masked_bins(F, T, zm)])
        sat, toi = pa_params(prec, F, kind)
        for mode, pk, p in MODES:
            ref, e_np = reference(prec, F, kind, mode)
            got = pu.fft(prec, F, variant, X, masked=masked, pa=pk, sat=sat, p=p, toi=toi)
            assert np.all(np.isfinite(got.view(pu.rdtype(prec))))
            ok, l2, mx = within(got, ref, e_np)
            print(f"PROBE_FFT|{_id(inst)}|T={T}|kind={fft_kind}|{kind}|{mode}|l2={l2.max():.3e}|e_np_l2={e_np[0].max():.3e}"
                  f"|ratio_l2={np.max(l2 / e_np[0]):.2f}|mx={mx.max():.3e}|e_np_mx={e_np[1].max():.3e}"
                  f"|ratio_mx={np.max(mx / e_np[1]):.2f}")
            if not ok:
                failures.append((kind, mode, float(np.max(l2 / e_np[0])), float(np.max(mx / e_np[1]))))
    assert not failures, f"{_id(inst)}: (input, PA, l2 / e_np, max-abs / e_np) beyond {FACTOR}: {failures}"


@gpu
def test_identity_round_trip_returns_F_times_the_input():
    """No PA: the two un-normalised transforms return F X (a check of the probe's own layout
    handling that needs no reference FFT)."""
    for prec, F, variant in [(0, 128, 0), (0, 2048, 0), (0, 8192, 0), (1, 1024, 3)]:
        X, _ = make_input(prec, F, "normal")
        got = pu.fft(prec, F, variant, X)
        l2, _ = pu.errors(got, np.array(X).astype(pu.CLD) * F)
        assert np.all(l2 < (1e-14 if prec == 0 else 1e-5)), (prec, F, l2)
