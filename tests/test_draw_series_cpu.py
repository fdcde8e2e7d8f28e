"""CPU bounds of the shortened series of the Rayleigh channel draws (csrc/tuning.h MIMO_P1_LN_DEG,
MIMO_BM_LN_DEG, MIMO_BM_SIN_DEG; csrc/real.h ln_unit / ln_unit_parts / sincos_lut DEG).

The float64 forms are restated operation by operation, as tests/test_pass1_logsum_cpu.py does
(whose table, sample, weights and fma() are used here), and set against long double (x87 extended,
eps 1.1e-19).  The references do not contain the series under test: the logarithm's is the
table's -ln c_i as stored plus log1p(t) and e ln 2 in long double, the sine's and cosine's are
the functions themselves of the angle word.

1. Pass 1 (Channel::power_acc): the three-sum form of sum_a c_a ln u_a with log1p to t^4, on that
   file's 10^6 words and config-2 weights.  Its largest error against the long-double sum must not
   exceed that of the per-draw form with the full series (the bar MIMO_P1_SUMS3 was held to: 7.31
   units of the float64 spacing at the sum).  The t^5 and t^6 terms are below 2e-16 each, the
   spacing at the sum of about 64 is 1.4e-14.
2. Array pass (Channel::normals_w): one log with log1p to t^5 stays within 2 units of its last
   place (it goes under sqrt_n1, itself 2^-47.8).
3. The sine to phi^5 and the cosine to phi^6, then the angle sum with the table's (cos, sin): both
   results within 2 units of the last place of the larger of |sin| and |cos|, over 10^6 random
   angle words and the words i 2^24 +- 2^23 (the residual's ends, |phi| = pi / 256, where the
   dropped phi^7 term is largest, at every table index).

Measured: 1. t^4 three sums max 4.138 (mean 0.735), per-draw full series 7.308; 2. t^5 max 1.685
(t^6 1.000); 3. sin 1.372, cos 1.379 (phi^7: 1.372, 1.376)."""
import numpy as np

from test_pass1_logsum_cpu import LD, LN2_HI, LN2_LO, N_ANT, config2_weights, fma, ln_parts

Q_ALL = (-1.0 / 6, 1.0 / 5, -1.0 / 4, 1.0 / 3, -0.5)  # real.h log1p_series: Horner from the DEG's term down


def log1p_series(t, deg):
    """real.h log1p_series<deg>: q by Horner in t from the t^deg term's coefficient, then t + t^2 q;
    to t^4 as t + u ((t / 3 - 1/2) - u / 4) with u = t^2."""
    if deg == 4:
        u = t * t
        return fma(u, fma(u, -0.25, fma(t, 1.0 / 3, -0.5)), t)
    coef = Q_ALL[6 - deg:]
    q = np.full_like(t, coef[0])
    for k in coef[1:]:
        q = fma(q, t, k)
    return fma(t * t, q, t)


def _sample():
    rng = np.random.default_rng(20482)
    return rng.integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).reshape(-1, N_ANT)


def _ln_terms(w):
    tab, poly6, e, m, c = ln_parts(w)
    t = fma(m, c, -1.0)
    np.testing.assert_array_equal(log1p_series(t, 6), poly6)  # the full series is ln_unit's as it was
    t_ld = m.astype(LD) * c.astype(LD) - LD(1)
    ref = tab.astype(LD) + np.log1p(t_ld) + e.astype(LD) * (LD(LN2_HI) + LD(LN2_LO))
    return tab, t, e, ref


def test_pass1_three_sums_to_t4():
    w = _sample()
    cw = config2_weights()
    tab, t, e, ln_ref = _ln_terms(w)
    ref = (cw.astype(LD) * ln_ref).sum(axis=1)
    poly6, poly4 = log1p_series(t, 6), log1p_series(t, 4)
    n = w.shape[0]
    nrm, T, P, E = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for a in range(N_ANT):
        ln = fma(e[:, a], LN2_HI, tab[:, a]) + fma(e[:, a], LN2_LO, poly6[:, a])
        nrm = fma(cw[a], ln, nrm)
        T = fma(cw[a], tab[:, a], T)
        P = fma(cw[a], poly4[:, a], P)
        E = fma(cw[a], e[:, a], E)
    sums3 = fma(E, LN2_HI, T) + fma(E, LN2_LO, P)
    sp = np.spacing(np.abs(ref).astype(np.float64)).astype(LD)
    err_old = np.asarray(np.abs(nrm.astype(LD) - ref) / sp, np.float64)
    err_new = np.asarray(np.abs(sums3.astype(LD) - ref) / sp, np.float64)
    print(f"DRAW_SERIES|pass1|per-draw t^6 max={err_old.max():.3f}|three sums t^4 max={err_new.max():.3f} "
          f"mean={err_new.mean():.3f}")
    assert ref.min() > 0 and np.all(np.isfinite(sums3))
    assert err_new.max() <= err_old.max()


def test_draw_log_to_t5():
    w = _sample()
    tab, t, e, ref = _ln_terms(w)
    sp = np.spacing(np.abs(ref).astype(np.float64)).astype(LD)
    err = {}
    for deg in (6, 5):
        ln = fma(e, LN2_HI, tab) + fma(e, LN2_LO, log1p_series(t, deg))  # real.h ln_unit
        err[deg] = float(np.asarray(np.abs(ln.astype(LD) - ref) / sp, np.float64).max())
    print(f"DRAW_SERIES|log|t^6 max={err[6]:.3f}|t^5 max={err[5]:.3f}")
    assert np.all(ref < 0)
    assert err[5] <= 2.0


H = 1.4629180792671596e-09  # real.h sincos_lut: 2 pi 2^-32 and the coefficients as the compiler folds them
H2 = H * H
PS7, PS5, PS3 = -(H2 * H2 * H2 * H) / 5040, (H2 * H2 * H) / 120, -(H2 * H) / 6
PC6, PC4, PC2 = -(H2 * H2 * H2) / 720, (H2 * H2) / 24, -H2 / 2


def _sincos_ld(num, den):
    """(sin, cos)(2 pi num / den) in long double for integers 0 <= num < den, den a multiple of 8:
    the nearest eighth of a revolution taken off exactly, the angle sum with its exact pair."""
    pi = LD(4) * np.arctan(LD(1))
    o = (8 * num + den // 2) // den  # nearest eighth, 0..8
    r = (num - o * (den // 8)).astype(LD) / LD(den)  # in [-1/16, 1/16], exact
    s, c = np.sin(LD(2) * pi * r), np.cos(LD(2) * pi * r)
    h = np.sqrt(LD(0.5))
    oc = np.array([1, h, 0, -h, -1, -h, 0, h, 1], LD)[o]
    os_ = np.array([0, h, 1, h, 0, -h, -1, -h, 0], LD)[o]
    return os_ * c + oc * s, oc * c - os_ * s


def sincos_lut(w, deg):
    """real.h sincos_lut<deg>(w) in float64, operation by operation."""
    w = w.astype(np.int64)
    i = ((w + 0x800000) >> 24) & 255
    f = (((w & 0xFFFFFF) ^ 0x800000) - 0x800000).astype(np.float64)  # the low 24 bits, sign-extended
    ts, tc = _sincos_ld(np.arange(256), 256)  # csrc/host_tables.h lut64_table, entries [512, 768)
    ts, tc = np.asarray(ts, np.float64), np.asarray(tc, np.float64)
    z = f * f  # exact
    ps = np.full_like(z, PS5)
    if deg == 7:
        ps = fma(z, PS7, PS5)
    ps = fma(ps, z, PS3)
    ps = fma(ps, z, H)
    s = f * ps
    pc = fma(z, PC6, PC4)
    pc = fma(pc, z, PC2)
    c = fma(z, pc, 1.0)
    cx, cy = tc[i], ts[i]
    return fma(cy, c, cx * s), fma(cx, c, -(cy * s))


def test_sine_to_phi5():
    rng = np.random.default_rng(20482)
    ends = np.arange(256, dtype=np.int64) << 24
    w = np.concatenate([rng.integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.int64),
                        (ends + (1 << 23)) % (1 << 32), (ends - (1 << 23)) % (1 << 32)])
    rs, rc = _sincos_ld(w, 1 << 32)
    sp = np.spacing(np.maximum(np.abs(rs), np.abs(rc)).astype(np.float64)).astype(LD)
    err = {}
    for deg in (7, 5):
        sn, cs = sincos_lut(w, deg)
        err[deg] = (float(np.asarray(np.abs(sn.astype(LD) - rs) / sp, np.float64).max()),
                    float(np.asarray(np.abs(cs.astype(LD) - rc) / sp, np.float64).max()))
    print(f"DRAW_SERIES|sincos|phi^7 max sin={err[7][0]:.3f} cos={err[7][1]:.3f}"
          f"|phi^5 max sin={err[5][0]:.3f} cos={err[5][1]:.3f}")
    assert w.size == 10 ** 6 + 512
    assert max(err[5]) <= 2.0
