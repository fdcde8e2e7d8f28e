"""CPU check of pass 1's weighted log sum in three running sums (csrc/tuning.h MIMO_P1_SUMS3).

Pass 1 of the perfect-CSI Rayleigh instances forms the MRT norm of a slot as
sum_a c_a ln u_a, c_a = -ant_rel_a^2, u_a = (w_a + 0.5) 2^-32 for the radius word w_a of antenna a
(csrc/philox.h bm_log).  real.h ln_unit gives ln u = tab + poly + e ln 2 (the table's -ln c_i, the
log1p polynomial, the exponent; ln 2 in a high and a low part).  Two float64 forms of the sum:

  present   per draw fma(e, ln2_hi, tab) + fma(e, ln2_lo, poly), then nrm = fma(c, ln, nrm)
  sums3     per draw T = fma(c, tab, T), P = fma(c, poly, P), E = fma(c, e, E); once per slot
            nrm = fma(E, ln2_hi, T) + fma(E, ln2_lo, P)              (real.h ln_unit_parts, ln_sum)

Both are restated here operation by operation on the table of csrc/host_tables.h lut64_table and
set against the same sum carried in long double (x87 extended, eps 1.1e-19) from the same
constants: the table's (c_i, -ln c_i) as stored, the polynomial's coefficients, ln 2 = hi + lo.
The sample is 10^6 random 32-bit words, 15,625 sums over the 64 antennas of the config-2 geometry
(oracle/refmath.py ula_positions; ant_rel = d_min / d_a as csrc/engine.hip forms it).  The new
form's largest error must not exceed the present form's.

fma(a, b, c) is float64(longdouble(a) longdouble(b) + longdouble(c)) here: the product keeps 64 of
its up to 106 bits, so this is the fused operation but for a double rounding in about one case in
2^11, and then by one unit of the last place of that intermediate; it meets both forms alike.

Measured on this sample (units of the float64 spacing at the reference sum, about 64):
present form max 7.31, mean 1.14; three sums max 4.14, mean 0.73."""
import numpy as np

from oracle import refmath as rm

LD = np.longdouble
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
Q = (-1.0 / 6, 1.0 / 5, -1.0 / 4, 1.0 / 3, -0.5)  # real.h ln_unit: q by Horner in t, then t + t^2 q
N_ANT = 64


def fma(a, b, c):
    return np.asarray(np.asarray(a, LD) * np.asarray(b, LD) + np.asarray(c, LD), np.float64)


def ln_table():
    """csrc/host_tables.h lut64_table, entries [0, 512): (c_i, -ln c_i); c_i = 1 / centre_i rounded
    to 12 bits, 1 for the top bucket."""
    i = np.arange(512)
    ctr = LD(0.5) + (i.astype(LD) + LD(0.5)) / LD(1024)
    fr, ex = np.frexp(LD(1) / ctr)
    c = np.ldexp(np.round(np.ldexp(fr, 12)), ex - 12).astype(np.float64)
    c[511] = 1.0
    return c, np.asarray(-np.log(c.astype(LD)), np.float64)


def ln_parts(w):
    """real.h ln_unit_parts<-32>((double)w + 0.5): (tab, poly, e) in float64, and t for the reference."""
    x = w.astype(np.float64) + 0.5  # exact
    m, e = np.frexp(x)  # m in [0.5, 1), as v_frexp_mant / v_frexp_exp
    hi = x.view(np.uint64) >> np.uint64(32)
    idx = ((hi >> np.uint64(11)) & np.uint64(511)).astype(np.int64)
    c, tab = ln_table()
    t = fma(m, c[idx], -1.0)
    q = np.full_like(t, Q[0])
    for k in Q[1:]:
        q = fma(q, t, k)
    poly = fma(t * t, q, t)
    return tab[idx], poly, (e - 32).astype(np.float64), m, c[idx]


def ld_ln(m, c, tab, e):
    """The same logarithm in long double from the same constants."""
    t = m.astype(LD) * c.astype(LD) - LD(1)
    q = np.full_like(t, LD(Q[0]))
    for k in Q[1:]:
        q = q * t + LD(k)
    return tab.astype(LD) + (t + t * t * q) + e.astype(LD) * (LD(LN2_HI) + LD(LN2_LO))


def config2_weights():
    tx = rm.ula_positions(N_ANT, 3.5e9, 0.5, 15.0)
    d = np.sqrt(((np.asarray(tx, np.float64) - np.array([212.0, 212.0, 1.5])) ** 2).sum(axis=1))
    ant_rel = d.min() / d
    return -(ant_rel * ant_rel)  # philox.h bm_c<double>(sa * sa)


def test_three_sums_no_worse_than_present_form():
    rng = np.random.default_rng(20482)
    w = rng.integers(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32).reshape(-1, N_ANT)
    cw = config2_weights()
    assert cw.shape == (N_ANT,) and np.all(cw < 0) and np.all(cw >= -1.0)
    tab, poly, e, m, c = ln_parts(w)
    ref = (cw.astype(LD) * ld_ln(m, c, tab, e)).sum(axis=1)

    nrm = np.zeros(w.shape[0])
    T, P, E = np.zeros(w.shape[0]), np.zeros(w.shape[0]), np.zeros(w.shape[0])
    for a in range(N_ANT):
        ln = fma(e[:, a], LN2_HI, tab[:, a]) + fma(e[:, a], LN2_LO, poly[:, a])
        nrm = fma(cw[a], ln, nrm)
        T = fma(cw[a], tab[:, a], T)
        P = fma(cw[a], poly[:, a], P)
        E = fma(cw[a], e[:, a], E)
    sums3 = fma(E, LN2_HI, T) + fma(E, LN2_LO, P)

    sp = np.spacing(np.abs(ref).astype(np.float64)).astype(LD)
    err_old = np.asarray(np.abs(nrm.astype(LD) - ref) / sp, np.float64)
    err_new = np.asarray(np.abs(sums3.astype(LD) - ref) / sp, np.float64)
    print(f"PASS1_LOGSUM|n_words={w.size}|present max={err_old.max():.3f} mean={err_old.mean():.3f}"
          f"|sums3 max={err_new.max():.3f} mean={err_new.mean():.3f}")
    assert ref.min() > 0 and np.all(np.isfinite(sums3))
    assert err_new.max() <= err_old.max()
