"""The host-built tables the trial kernels run on (csrc/host_tables.h, read back through
libmimo_probe's host-only entry points: no GPU): FFT twiddles and cot-tan constants against the
long-double exp, the Box-Muller tables against their definition, the per-point Bussgang-gain
fits against the 40-digit formula -- and, on the CPU, that the float64 FFT bound of
tests/test_gpu_probe_fft.py has teeth: a table rounded through float32 breaks it."""
import numpy as np
import pytest

import probe_util as pu
from probe_util import CLD, LD

ULP1 = float(np.spacing(1.0))          # 2^-52
ULP1_F32 = float(np.spacing(np.float32(1.0)))


def _team(prec, F, variant=0):
    return pu.fft_info(prec, F, variant)[0]


def _stage_ref(F, P):
    e = pu.stage_exponents(F, P)
    return pu.ld_cis_rev(-e, np.full_like(e, F))


def _ct_ref(F, P):
    ang = pu.ct_angles(F, P)
    return pu.ld_cis_rev([a[0] for a in ang], [a[1] for a in ang])


def _comp_err(got, ref):
    """Largest component error |got - ref| (long double); twiddles have modulus 1, so the unit
    is ulp(1): a relative error per component means nothing next to a zero of cos or sin."""
    d = np.asarray(got, CLD) - ref
    return float(max(np.max(np.abs(d.real)), np.max(np.abs(d.imag))))


def _layouts():
    """(name, prec, table, [(offset, kind, F_sub, P)]) of every production FFT table."""
    out = []
    for prec in (0, 1):
        for F in pu.SIZES:
            T, _, kind = pu.fft_info(prec, F, 0)
            P = F // T
            if kind == 2:  # split: the F/2-point sub-transform's tables, then the radix-2 stage's (cos, tan)
                tab = pu.table("split", 0, F)
                n_st, n_ct = len(pu.stage_exponents(F // 2, P)), len(pu.ct_angles(F // 2, P))
                out.append((f"split F={F}", prec, tab, [(0, "tw", F // 2, P), (n_st, "ct", F // 2, P),
                                                         (n_st + n_ct, "r2", F, 0)]))
                assert np.array_equal(tab, pu.table("team", 0, F))  # what the engine uploads as `tw`
                continue
            tab = pu.table("team", prec, F)
            out.append((f"team prec={prec} F={F}", prec, tab,
                        [(0, "tw", F, P), (len(pu.stage_exponents(F, P)), "ct", F, P)]))
            if kind == 1:  # wave-split: sub-transform stages, exp(-j 2 pi n / F), sub-transform cot-tan
                FW = F // (T // 64)
                n_st = len(pu.stage_exponents(FW, P))
                out.append((f"wave F={F}", prec, pu.table("wave", prec, F),
                            [(0, "tw", FW, P), (n_st, "full", F, 0), (n_st + F, "ct", FW, P)]))
            if prec == 1 and F >= 1024:
                Pa = F // _team(1, F, 2)
                out.append((f"team_alt F={F}", 1, pu.table("team_alt", 1, F),
                            [(0, "tw", F, Pa), (len(pu.stage_exponents(F, Pa)), "ct", F, Pa)]))
    return out


@pytest.fixture(scope="module")
def layouts():
    return _layouts()


def test_table_lengths_match_the_layout(layouts):
    for name, prec, tab, parts in layouts:
        n = 0
        for off, kind, Fs, P in parts:
            assert off == n, name
            n += {"tw": lambda: len(pu.stage_exponents(Fs, P)), "ct": lambda: len(pu.ct_angles(Fs, P)),
                  "full": lambda: Fs, "r2": lambda: Fs // 2}[kind]()
        assert n == tab.size, (name, n, tab.size)


def test_twiddle_entries_within_one_ulp_of_long_double(layouts):
    """Every exp(-j 2 pi e / F) entry (stage blocks, the wave-split FFT's inter-step twiddles):
    both components within 1 ulp(1) of the long-double value, in the table's own precision."""
    worst = {}
    for name, prec, tab, parts in layouts:
        ulp = ULP1 if prec == 0 else ULP1_F32
        for off, kind, Fs, P in parts:
            if kind == "tw":
                ref = _stage_ref(Fs, P)
            elif kind == "full":
                ref = pu.ld_cis_rev(-np.arange(Fs), np.full(Fs, Fs))
            else:
                continue
            err = _comp_err(tab[off:off + ref.size], ref) / ulp
            worst[f"{name} {kind}"] = err
    print({k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


def test_cot_tan_pairs(layouts):
    """Every (c, t) = (cos a, tan a): finite, and c t within 1 ulp(1) of sin a (the product is
    what the butterflies' FMAs form; at a quarter turn c is 1e-20-sized and t its huge inverse)."""
    worst = {}
    for name, prec, tab, parts in layouts:
        ulp = ULP1 if prec == 0 else ULP1_F32
        for off, kind, Fs, P in parts:
            if kind == "ct":
                ref = _ct_ref(Fs, P)
            elif kind == "r2":
                ref = pu.ld_cis_rev(-np.arange(Fs // 2), np.full(Fs // 2, Fs))
            else:
                continue
            if ref.size == 0:
                continue
            c, t = tab[off:off + ref.size].real, tab[off:off + ref.size].imag
            assert np.all(np.isfinite(c)) and np.all(np.isfinite(t)), name
            assert np.all(c != 0), name
            ct = c.astype(LD) * t.astype(LD)
            worst[f"{name} {kind}"] = max(float(np.max(np.abs(ct - ref.imag))), float(np.max(np.abs(c.astype(LD) - ref.real)))) / ulp
    print({k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


def _mp():
    try:
        import mpmath
    except ImportError:
        return None
    mpmath.mp.dps = 40
    return mpmath.mp


def test_lut64_pairs():
    """real.h's tables: (c_i, -ln c_i) with c_i of at most 12 significant bits and c = 1 for the
    top bucket, -ln c_i correctly rounded; (cos, sin)(2 pi i / 256) correctly rounded."""
    tab = pu.table("lut64")
    assert tab.size >= 768
    c, l = tab[:512].real, tab[:512].imag
    m, _ = np.frexp(c)
    assert np.all(m * 4096 == np.round(m * 4096)), "c_i has more than 12 significant bits"
    assert c[511] == 1.0 and l[511] == 0.0
    mp = _mp()
    if mp is not None:
        want_l = np.array([float(-mp.log(mp.mpf(float(ci)))) for ci in c])
        ang = [2 * mp.pi * i / 256 for i in range(256)]
        want_c = np.array([float(mp.cos(a)) for a in ang])
        want_s = np.array([float(mp.sin(a)) for a in ang])
        # the exact zeros of the circle (mpmath's pi is rounded: cos(pi/2) comes out 1e-41)
        want_c[[64, 192]] = 0.0
        want_s[[0, 128]] = 0.0
    else:  # long double: correctly rounded to double except at a near-tie of the 64-bit value
        want_l = np.asarray(-np.log(c.astype(LD)), np.float64)
        a = 2 * pu.LD_PI * np.arange(256, dtype=LD) / 256
        want_c, want_s = np.asarray(np.cos(a), np.float64), np.asarray(np.sin(a), np.float64)
    np.testing.assert_array_equal(l, want_l)
    cs = tab[512:768]
    # the table stores what long-double cos / sin give at the rounded pi: 1e-19-sized values
    # in place of the circle's exact zeros are within half an ulp(1) and are accepted as such
    zc, zs = want_c == 0, want_s == 0
    np.testing.assert_array_equal(cs.real[~zc], want_c[~zc])
    np.testing.assert_array_equal(cs.imag[~zs], want_s[~zs])
    assert np.all(np.abs(cs.real[zc]) < ULP1 / 2) and np.all(np.abs(cs.imag[zs]) < ULP1 / 2)


def _fma64(a, x, c):
    return np.asarray(a.astype(LD) * x.astype(LD) + LD(c), np.float64)


def ld_erfc(g):
    """erfc in long double for g > 0 (alpha, of order 1, needs ~1e-19 absolute): up to g = 3 as
    1 - erf by the all-positive series erf(g) = 2 / sqrt(pi) e^{-g^2} sum_n 2^n g^(2n+1) /
    (1 3 ... (2n+1)) (no cancellation); above by the continued fraction e^{-g^2} / sqrt(pi) /
    (g + (1/2) / (g + 1 / (g + (3/2) / (g + ...)))), all terms positive, evaluated backwards."""
    g = np.asarray(g, LD)
    gs = np.minimum(g, LD(3))
    term = gs.copy()
    tot = gs.copy()
    for n in range(1, 120):
        term = term * (2 * gs * gs) / LD(2 * n + 1)
        tot = tot + term
    small = LD(1) - 2 / np.sqrt(pu.LD_PI) * np.exp(-gs * gs) * tot
    gb = np.maximum(g, LD(3))
    k = gb.copy()
    for n in range(300, 0, -1):
        k = gb + LD(n) / 2 / k
    big = np.exp(-gb * gb) / (np.sqrt(pu.LD_PI) * k)
    return np.where(g <= 3, small, big)


def alpha_ref(g0sq, x):
    """alpha(g0^2 / (1 + x)) = 1 - e^{-g^2} + sqrt(pi) / 2 g erfc(g) (modulation.py:178-189) as
    long doubles: by mpmath at 30 digits where it is importable, else in long double."""
    mp = _mp()
    x = np.asarray(x, np.float64)
    if mp is None:
        g2 = LD(g0sq) / (LD(1) + x.astype(LD))
        g = np.sqrt(g2)
        return LD(1) - np.exp(-g2) + np.sqrt(pu.LD_PI) / 2 * g * ld_erfc(g)
    sqpi2 = mp.sqrt(mp.pi) / 2
    ref = np.empty(x.size, LD)
    for i, xi in enumerate(x):
        g2 = mp.mpf(g0sq) / (1 + mp.mpf(float(xi)))
        g = mp.sqrt(g2)
        v = 1 - mp.exp(-g2) + sqpi2 * g * mp.erfc(g)
        hi = float(v)
        ref[i] = LD(hi) + LD(float(v - hi))
    return ref


def test_long_double_alpha_reference_agrees_with_mpmath():
    """The fallback of alpha_ref (no mpmath) against the 40-digit formula, where both exist."""
    mp = _mp()
    if mp is None:
        pytest.skip("mpmath is what this compares with")
    x = np.linspace(-0.25, 0.25, 41)
    for ibo_db in (-5.0, 0.0, 7.0, 15.0, 30.0):
        g0sq = 10.0 ** (ibo_db / 10.0)
        g2 = LD(g0sq) / (LD(1) + x.astype(LD))
        g = np.sqrt(g2)
        ld = LD(1) - np.exp(-g2) + np.sqrt(pu.LD_PI) / 2 * g * ld_erfc(g)
        assert float(np.max(np.abs((ld - alpha_ref(g0sq, x)) / ld))) < 1e-18, ibo_db


@pytest.mark.parametrize("ibo_db", [-5.0, 0.0, 3.0, 7.0, 15.0, 30.0])
def test_fit_alpha_against_the_formula(ibo_db):
    """host_tables.h fit_alpha: the degree-18 Horner sum in float64 (the kernel's FMA
    recurrence) within the comment's 1.6e-16 relative of alpha(g0^2 / (1 + x)), the degree-8
    sum in float32 within its 1e-7, over 10^4 x in [-xlim, xlim]."""
    g0sq = 10.0 ** (ibo_db / 10.0)
    amono, apoly, xlim = pu.alpha_fit(g0sq)
    assert xlim == 0.25
    x = np.concatenate([[-xlim, 0.0, xlim], np.random.default_rng(int(ibo_db * 10) + 77).uniform(-xlim, xlim, 9997)])
    ref = alpha_ref(g0sq, x)
    acc = np.full(x.size, amono[18])
    for k in range(17, -1, -1):
        acc = _fma64(acc, x, amono[k])
    e64 = float(np.max(np.abs((acc.astype(LD) - ref) / ref)))
    x32 = x.astype(np.float32)
    ref32 = alpha_ref(g0sq, x32)  # the float32 kernel sees the float32 x: the formula at that x
    a32 = np.full(x.size, np.float32(apoly[8]))
    for i in range(7, -1, -1):  # fmaf: exact product and sum in float64, one rounding to float32
        a32 = (a32.astype(np.float64) * x32.astype(np.float64) + np.float64(np.float32(apoly[i]))).astype(np.float32)
    e32 = float(np.max(np.abs((a32.astype(LD) - ref32) / ref32)))
    print(f"IBO {ibo_db:+.0f} dB: degree-18 float64 {e64:.3e}, degree-8 float32 {e32:.3e}")
    assert e64 <= 1.6e-16, e64
    assert e32 <= 1e-7, e32


# ---------------------------------------------------------------- teeth of the float64 bound
def test_float32_rounded_table_breaks_the_float64_bound():
    """The bound of tests/test_gpu_probe_fft.py (16 x NumPy's own float64 error against long
    double) on the CPU: the production float64 cot-tan constants of the F 4096 team's radix-16
    stage through the NumPy restatement of dft16_ct (tests/test_fft_ct.py) stay inside it; the
    same constants rounded through float32 -- a float table in a float64 kernel -- break it."""
    import test_fft_ct as ct
    F, T = 4096, _team(0, 4096)
    P = F // T
    assert P == 16 and pu.fft_bits(F, P, 1) == 4
    NS = 1 << pu.fft_bits_before(F, P, 1)
    tab = pu.table("team", 0, F)
    off = len(pu.stage_exponents(F, P))
    rows = tab[off:off + 8 * NS].reshape(8, NS)
    rng = np.random.default_rng(4096)
    k = np.arange(16)
    got, got32, ref, ynp = [], [], [], []
    for jm in range(NS):
        v = rng.standard_normal(16) + 1j * rng.standard_normal(16)
        zc = [(rows[q, jm].real, rows[q, jm].imag) for q in range(8)]
        zc32 = [(float(np.float32(c)), float(np.float32(t))) for c, t in zc]
        got.append(ct.dft16_ct(-1, v, zc))
        got32.append(ct.dft16_ct(-1, v, zc32))
        z = pu.ld_cis_rev(-jm * k, np.full(16, 16 * NS))  # z^r, z = exp(-j 2 pi jm / (R NS))
        ref.append(pu.ld_fft(z * v.astype(CLD), -1))
        ynp.append(np.fft.fft(np.exp(-2j * np.pi * jm * k / (16 * NS)) * v))
    got, got32, ref, ynp = (np.concatenate(a) for a in (got, got32, ref, ynp))
    (e_np,), _ = pu.errors(ynp[None], ref[None])
    (e_ok,), _ = pu.errors(got[None], ref[None])
    (e_32,), _ = pu.errors(got32[None], ref[None])
    print(f"e_np {e_np:.3e}  float64 table {e_ok:.3e}  float32-rounded table {e_32:.3e}")
    assert e_ok <= 16 * e_np
    assert e_32 > 16 * e_np
    assert e_32 > 1e3 * 16 * e_np  # not a near miss: orders of magnitude outside
