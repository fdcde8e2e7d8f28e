"""The float64 primitives of csrc/real.h (table-driven ln / sincos, Newton square roots, the
integer-hardness Rapp root) and pa_block of csrc/pa.h on the device, through
libmimo_probe, against long double -- at the bounds the code comments state:

  ln_unit <= 1.3 ulp; sincos_lut, sincos_rev_lut <= 1.5 x 2^-53 absolute (next to a zero of
  sin a relative error means nothing); sqrt_n1, rsq_n1 <= 2^-47.5 relative; the integer-hardness
  Rapp root rpow_neg_inv <= 0.75 ulp.  Three of these were first measured
  on the device by this file and the comments corrected to the measurement: ln_unit said 1.1 ulp
  (measured 1.243 at w = 0x483f4f6b), the one-step square roots ~2^-49 (measured 2^-47.83:
  4.0e-15), the Rapp root 0.7 ulp (measured 0.708 for N = 6).  rsq_r(double) carries no claim:
  after its two Newton steps the residual of the 2^-25 seed is 2^-97, what is left is the last
  FMA's rounding (0.5 ulp) and the roundings of 0.5 x and of (0.5 x) y inside the correction,
  each weighted 1/2: <= 2 ulp.

About 2 10^5 inputs per function in one launch each.  The measured maxima are recorded in
profiles/r07/probe/accuracy.md."""
import numpy as np
import pytest

import probe_util as pu
from probe_util import LD

pytestmark = pytest.mark.gpu

N_RANDOM = 150_000
U53 = 2.0 ** -53


def rel_ulp(got, ref):
    return pu.ulp_err(got, ref)


def words():
    """uint32 words: random, every ln_unit bucket boundary +-1 in every binade, all w < 1024,
    0 and 0xFFFFFFFF, k 2^30 and k 2^24 (+-1), the sincos index's rounding boundaries
    k 2^24 + 2^23 (+-1) and the wrap w >= 0xFF800000."""
    rng = np.random.default_rng(20)
    parts = [rng.integers(0, 1 << 32, N_RANDOM, dtype=np.uint64), np.arange(1024, dtype=np.uint64)]
    d = np.array([-1, 0, 1], np.int64)
    for k in range(9, 32):  # x = w + 0.5 in [2^k, 2^(k+1)): bucket i starts at 2^k + i 2^(k-9)
        b = (1 << k) + np.arange(513, dtype=np.int64) * (1 << (k - 9))
        parts.append((b[:, None] + d).ravel())
    for step, n in ((1 << 30, 5), (1 << 24, 257)):
        b = np.arange(n, dtype=np.int64) * step
        parts.append((b[:, None] + d).ravel())
    b = np.arange(256, dtype=np.int64) * (1 << 24) + (1 << 23)
    parts.append((b[:, None] + d).ravel())
    parts.append(np.arange(0xFF800000 - 2, 0xFF800000 + 3, dtype=np.int64))
    parts.append(rng.integers(0xFF800000, 1 << 32, 4096, dtype=np.uint64))
    w = np.concatenate([np.asarray(p, np.int64) for p in parts])
    w = np.unique(w[(w >= 0) & (w < (1 << 32))])
    assert w[0] == 0 and w[-1] == 0xFFFFFFFF
    return w.astype(np.uint32)


def test_ln_unit():
    w = words()
    got = pu.math("ln_unit", w)
    ref = np.log((w.astype(LD) + LD(0.5)) * LD(2.0) ** -32)
    err = rel_ulp(got, ref)
    i = int(np.argmax(err))
    print(f"PROBE_MATH|ln_unit|n={w.size}|max_ulp={err[i]:.3f}|at_w={int(w[i]):#x}|claim=1.3")
    assert np.all(got < 0)
    assert err[i] <= 1.3, (err[i], hex(int(w[i])))


def test_sincos_lut():
    w = words()
    sn, cs = pu.math("sincos_lut", w)
    a = 2 * pu.LD_PI * (w.astype(LD) * LD(2.0) ** -32)
    es = np.asarray(np.abs(sn.astype(LD) - np.sin(a)), np.float64) / U53
    ec = np.asarray(np.abs(cs.astype(LD) - np.cos(a)), np.float64) / U53
    print(f"PROBE_MATH|sincos_lut|n={w.size}|max_sin={es.max():.3f}|max_cos={ec.max():.3f}|unit=2^-53|claim=1.5")
    assert es.max() <= 1.5 and ec.max() <= 1.5, (es.max(), ec.max())


def test_sincos_rev_lut():
    rng = np.random.default_rng(21)
    k = rng.integers(-(1 << 28), 1 << 28, 20000)
    r = np.concatenate([
        rng.uniform(-2.0 ** 20, 2.0 ** 20, N_RANDOM // 2), rng.uniform(-1, 1, N_RANDOM // 2),
        k / 256.0, (k[:5000] % (1 << 22)) / 4.0, (2 * k[:5000] + 1) / 512.0,             # table points, zeros, rint ties
        np.nextafter(k[:5000] / 256.0, np.inf), np.nextafter(k[:5000] / 256.0, -np.inf),
        -np.abs(rng.uniform(0, 2.0 ** 20, 5000)), 10.0 ** rng.uniform(-300, 0, 5000), [0.0, -0.0, 0.25, -0.25, 0.5],
        [np.nextafter(2.0 ** 20, 0), -np.nextafter(2.0 ** 20, 0)]])
    assert np.all(np.abs(r) < 2.0 ** 20)
    sn, cs = pu.math("sincos_rev_lut", r)
    rl = r.astype(LD)
    a = 2 * pu.LD_PI * (rl - np.floor(rl))  # exact: |r| < 2^20 leaves 33 fraction bits in 64
    es = np.asarray(np.abs(sn.astype(LD) - np.sin(a)), np.float64) / U53
    ec = np.asarray(np.abs(cs.astype(LD) - np.cos(a)), np.float64) / U53
    print(f"PROBE_MATH|sincos_rev_lut|n={r.size}|max_sin={es.max():.3f}|max_cos={ec.max():.3f}|unit=2^-53|claim=1.5")
    assert es.max() <= 1.5 and ec.max() <= 1.5, (es.max(), ec.max())


def positives():
    rng = np.random.default_rng(22)
    x = np.ldexp(rng.uniform(0.5, 1.0, N_RANDOM), rng.integers(-100, 101, N_RANDOM))
    p2 = 2.0 ** np.arange(-100, 101)
    return np.concatenate([x, p2, np.nextafter(p2, np.inf), np.nextafter(p2, 0), [2.0, 3.0, 4.0, 0.1]])


@pytest.mark.parametrize("fn,claim_rel,claim_ulp", [("sqrt_n1", 2.0 ** -47.5, None), ("rsq_n1", 2.0 ** -47.5, None),
                                                    ("rsq_r", None, 2.0)])
def test_square_roots(fn, claim_rel, claim_ulp):
    x = positives()
    got = pu.math(fn, x)
    ref = np.sqrt(x.astype(LD))
    if fn != "sqrt_n1":
        ref = LD(1) / ref
    rel = np.asarray(np.abs((got.astype(LD) - ref) / ref), np.float64)
    ulp = rel_ulp(got, ref)
    print(f"PROBE_MATH|{fn}|n={x.size}|max_rel={rel.max():.3e}|max_rel_log2={np.log2(rel.max()):.2f}|max_ulp={ulp.max():.3f}"
          f"|claim={'2^-47.5' if claim_rel else '2 ulp'}")
    if claim_rel is not None:
        assert rel.max() <= claim_rel, (rel.max(), np.log2(rel.max()))
    else:
        assert ulp.max() <= claim_ulp, ulp.max()


@pytest.mark.parametrize("N", [4, 6])
def test_rpow_neg_inv(N):
    rng = np.random.default_rng(23 + N)
    t = np.concatenate([10.0 ** rng.uniform(-12, 6, N_RANDOM), 10.0 ** np.arange(-12.0, 6.5, 0.5), [0.0, 1.0, 1e6]])
    y = 1.0 + t
    got = pu.math(f"rpow{N}", y)
    ref = np.power(y.astype(LD), LD(-1) / LD(N))
    ulp = rel_ulp(got, ref)
    i = int(np.argmax(ulp))
    print(f"PROBE_MATH|rpow_neg_inv<{N}>|n={y.size}|max_ulp={ulp[i]:.3f}|at_y={y[i]!r}|claim=0.75")
    assert ulp[i] <= 0.75, (ulp[i], y[i])


# ---------------------------------------------------------------- PA block
PA_CASES = [("softlim", pu.PA_SOFTLIM, 0.0), ("rapp2", pu.PA_RAPP, 2.0), ("rapp3", pu.PA_RAPP, 3.0),
            ("rapp4", pu.PA_RAPP, 4.0), ("rapp5", pu.PA_RAPP, 5.0), ("rapp2.5", pu.PA_RAPP, 2.5), ("toi", pu.PA_TOI, 0.0)]


def pa_inputs(prec):
    """(x, sat, toi): magnitudes with |x|^2 / sat from 1e-12 to 1e6 at random phases, the axes,
    and exact zeros."""
    rt, ct = pu.rdtype(prec), pu.cdtype(prec)
    rng = np.random.default_rng(30 + prec)
    sat = float(rt(2.75))
    ratio = np.concatenate([10.0 ** rng.uniform(-12, 6, 60000), 10.0 ** np.arange(-12.0, 6.25, 0.25), [1.0]])
    ph = rng.uniform(0, 2 * np.pi, ratio.size)
    ph[-80:] = np.repeat([0.0, np.pi / 2, np.pi, -np.pi / 2], 20)
    x = (np.sqrt(ratio * sat) * np.exp(1j * ph)).astype(ct)
    x = np.concatenate([x, np.zeros(8, ct)])
    return x, sat, float(rt(0.05 / sat))


def sat_edge_inputs(prec):
    """|x|^2 exactly sat - 1 ulp, sat, sat + 1 ulp in the instance's own arithmetic
    (fma(re, re, im im)): re = 1, im^2 = k u with u = ulp(1), sat = 1 + 2 u."""
    rt, ct = pu.rdtype(prec), pu.cdtype(prec)
    u = float(np.spacing(rt(1.0)))
    im = np.array([rt(np.sqrt(k * u)) for k in (1, 2, 3)], rt)
    pw = np.array([rt(LD(1) + LD(rt(v * v))) for v in im], rt)  # the fma's single rounding of 1 + fl(im^2)
    sat = rt(1.0 + 2 * u)
    assert pw[0] == np.nextafter(sat, rt(0)) and pw[1] == sat and pw[2] == np.nextafter(sat, rt(4)), pw
    x = np.concatenate([(1.0 + 1j * im.astype(np.float64)), (im.astype(np.float64) + 1j), [0j]]).astype(ct)
    return x, float(sat), float(rt(0.05))


def pa_errors(got, x, kind, sat, p, toi, prec):
    """Relative error of the complex output against the long-double formula at the same
    (rounded) inputs, in units of the type's 2^-52 / 2^-23.  The third-order model
    x (1 - c |x|^2) cancels near c |x|^2 = 1, where no evaluation of the formula keeps a
    relative accuracy: its error is taken relative to the larger term, |x| max(1, c |x|^2)."""
    ref = pu.ld_pa(kind, x.astype(pu.CLD), sat, p, toi)
    scale = np.abs(ref)
    if kind == pu.PA_TOI:
        xl = x.astype(pu.CLD)
        scale = np.abs(xl) * np.maximum(LD(1), LD(toi) * np.abs(xl) ** 2)
    nz = scale > 0
    assert np.all(np.asarray(got)[~nz] == 0)
    eps = float(np.spacing(pu.rdtype(prec)(1.0)))
    return np.asarray(np.abs(got.astype(pu.CLD) - ref)[nz] / scale[nz], np.float64) / eps


def np_pa(x, kind, sat, p, toi):
    from oracle import refmath as rm
    rt = x.real.dtype.type
    if kind == pu.PA_SOFTLIM:
        return np.asarray(rm.soft_limiter(rt(sat), x), x.dtype)
    if kind == pu.PA_RAPP:
        return np.asarray(rm.rapp(rt(sat), rt(p), x), x.dtype)
    return np.asarray(rm.toi(rt(toi), x), x.dtype)


@pytest.mark.parametrize("cold_out", [0, 1])
@pytest.mark.parametrize("name,kind,p", PA_CASES)
def test_pa_block_float64(name, kind, p, cold_out):
    """Within 4 ulp relative: a handful of correctly rounded operations after a <= 1-ulp gain.

    Measured on an MI355X (units of 2^-52, both COLD_OUT forms alike): softlim 1.45, rapp2 1.21,
    rapp3 1.23, rapp4 1.37, rapp5 1.40, rapp2.5 1.45, toi 1.34.  The first measurement had the
    soft limiter at 17.5 (one Newton step on the v_rsq_f64 seed) and the general-hardness Rapp
    gain at 8.8 (p = 5) and 11.6 (p = 2.5; exp2 / log2 with the rounding of p log2 u): fixed in
    real.h rsq_h1 and pa.h pa_apply."""
    worst = 0.0
    for x, sat, toi in (pa_inputs(0), sat_edge_inputs(0)):
        got = pu.pa(0, cold_out, kind, x, sat, p, toi)
        worst = max(worst, float(pa_errors(got, x, kind, sat, p, toi, 0).max()))
    print(f"PROBE_PA|f64|{name}|cold_out={cold_out}|max_ulp={worst:.3f}|bound=4")
    assert worst <= 4.0, worst


@pytest.mark.parametrize("cold_out", [0, 1])
@pytest.mark.parametrize("name,kind,p", PA_CASES)
def test_pa_block_float32(name, kind, p, cold_out):
    """The float32 instance keeps the hardware approximations: within 16 x the error of the same
    formula evaluated by NumPy in float32 on the same inputs."""
    worst, worst_np = 0.0, 0.0
    for x, sat, toi in (pa_inputs(1), sat_edge_inputs(1)):
        got = pu.pa(1, cold_out, kind, x, sat, p, toi)
        worst = max(worst, float(pa_errors(got, x, kind, sat, p, toi, 1).max()))
        with np.errstate(all="ignore"):
            worst_np = max(worst_np, float(pa_errors(np_pa(x, kind, sat, p, toi), x, kind, sat, p, toi, 1).max()))
    print(f"PROBE_PA|f32|{name}|cold_out={cold_out}|max_ulp={worst:.3f}|numpy_float32_ulp={worst_np:.3f}|bound={16 * worst_np:.3f}")
    assert worst <= 16 * worst_np, (worst, worst_np)
