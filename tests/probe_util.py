"""Loader of libmimo_probe.so (csrc/probe.h) and the long-double reference the probe tests
compare it with: a recursive radix-2 FFT in np.clongdouble (x87 extended precision, eps
1.1e-19: three decimal digits below float64), the PA formulas of oracle/refmath.py restated in
long double, the two error metrics, and Python mirrors of the stage plan (csrc/team_fft.h)
that name the exponent of every entry of the production twiddle tables."""
import ctypes
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "m-mimo-ofdm-with-nonlinear-pa-sim_amd")
LIB_PATH = os.path.join(PKG, "libmimo_probe.so")

LD = np.longdouble
CLD = np.clongdouble
LD_PI = LD(4) * np.arctan(LD(1))
SIZES = (128, 256, 512, 1024, 2048, 4096, 8192)
PA_NONE, PA_SOFTLIM, PA_RAPP, PA_TOI = 0, 1, 2, 3
FN = {"ln_unit": 0, "sincos_lut": 1, "sincos_rev_lut": 2, "sqrt_n1": 3, "rsq_n1": 4, "rsq_r": 5, "rpow4": 6,
      "rpow6": 7}
TABLE = {"team": 0, "team_alt": 1, "wave": 2, "split": 3, "lut64": 4}


class ProbeError(RuntimeError):
    pass


_lib = None


def lib():
    """The probe library; a missing one is an error (never a skip): build it."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ProbeError(f"{LIB_PATH} not found: build it with `make -C {os.path.join(PKG, 'csrc')}`")
        L = ctypes.CDLL(LIB_PATH)
        vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
        sig = {
            "mimo_probe_last_error": (ctypes.c_char_p, []),
            "mimo_probe_fft_info": (i32, [i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(i32)]),
            "mimo_probe_fft": (i32, [i32, i32, i32, i32, i32, dbl, dbl, dbl, i32, vp, vp]),
            "mimo_probe_math": (i32, [i32, i64, vp, vp, vp]),
            "mimo_probe_pa": (i32, [i32, i32, i32, dbl, dbl, dbl, i64, vp, vp]),
            "mimo_probe_alpha_fit": (i32, [dbl, vp, vp, ctypes.POINTER(dbl)]),
            "mimo_probe_table": (i32, [i32, i32, i32, vp, ctypes.POINTER(i64)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise ProbeError(f"probe error {rc}: {lib().mimo_probe_last_error().decode()}")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def cdtype(prec):
    return np.complex128 if prec == 0 else np.complex64


def rdtype(prec):
    return np.float64 if prec == 0 else np.float32


def fft_instances():
    """(prec, F, variant) of every production FFT instance (probe.h)."""
    out = [(0, F, 0) for F in SIZES]
    for F in SIZES:
        out += [(1, F, v) for v in ((0, 1, 2, 3) if F >= 1024 else (0, 1))]
    return out


def fft_info(prec, F, variant):
    """(team size T, zero mask, kind) -- kind 0 team, 1 wave-split, 2 split."""
    t, zm, k = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_int32()
    _check(lib().mimo_probe_fft_info(prec, F, variant, ctypes.byref(t), ctypes.byref(zm), ctypes.byref(k)))
    return t.value, zm.value, k.value


def masked_bins(F, T, zero_mask):
    """Boolean [F]: the bins [T m, T (m + 1)) of the registers m in the mask."""
    keep = np.zeros(F, bool)
    for m in range(F // T):
        if (zero_mask >> m) & 1:
            keep[T * m:T * (m + 1)] = True
    return keep


def fft(prec, F, variant, x, masked=False, pa=PA_NONE, sat=0.0, p=0.0, toi=0.0):
    x = np.ascontiguousarray(x, cdtype(prec)).reshape(-1, F)
    out = np.empty_like(x)
    _check(lib().mimo_probe_fft(prec, F, variant, int(masked), pa, sat, p, toi, x.shape[0], _ptr(x), _ptr(out)))
    return out


def math(fn, x):
    """fn by name (FN); x: uint32 words for ln_unit / sincos_lut, float64 else.  One array, or
    (sin, cos) for the two sincos forms."""
    code = FN[fn]
    x = np.ascontiguousarray(x, np.uint32 if code <= 1 else np.float64)
    o0 = np.empty(x.size, np.float64)
    o1 = np.empty(x.size, np.float64) if code in (1, 2) else None
    _check(lib().mimo_probe_math(code, x.size, _ptr(x), _ptr(o0), _ptr(o1) if o1 is not None else None))
    return (o0, o1) if o1 is not None else o0


def pa(prec, cold_out, kind, x, sat=0.0, p=0.0, toi=0.0):
    x = np.ascontiguousarray(x, cdtype(prec)).ravel()
    out = np.empty_like(x)
    _check(lib().mimo_probe_pa(prec, int(cold_out), kind, sat, p, toi, x.size, _ptr(x), _ptr(out)))
    return out


def alpha_fit(g0sq):
    """(amono[19], apoly[9], xlim) of csrc/host_tables.h fit_alpha."""
    am, ap, xl = np.empty(19), np.empty(9), ctypes.c_double()
    _check(lib().mimo_probe_alpha_fit(g0sq, _ptr(am), _ptr(ap), ctypes.byref(xl)))
    return am, ap, xl.value


def table(kind, prec=0, F=0):
    """A production table as a complex array (pairs (x, y) -> x + j y)."""
    n = ctypes.c_int64(0)
    _check(lib().mimo_probe_table(TABLE[kind], prec, F, None, ctypes.byref(n)))
    buf = np.empty(n.value, cdtype(prec))
    _check(lib().mimo_probe_table(TABLE[kind], prec, F, _ptr(buf), ctypes.byref(n)))
    assert n.value == buf.size
    return buf


# ---------------------------------------------------------------- long-double reference
@functools.lru_cache(maxsize=None)
def _twiddles(n, sign):
    return np.exp(CLD(1j) * (LD(sign) * 2 * LD_PI * np.arange(n // 2, dtype=LD) / LD(n)))


def ld_fft(x, sign=-1):
    """Un-normalised DFT along the last axis, sum_n x[n] exp(sign j 2 pi n k / N), in long
    double by recursive radix-2 decimation in time (N a power of two)."""
    x = np.asarray(x, CLD)
    n = x.shape[-1]
    if n == 1:
        return x.copy()
    e, o = ld_fft(x[..., 0::2], sign), ld_fft(x[..., 1::2], sign)
    o = o * _twiddles(n, sign)
    return np.concatenate([e + o, e - o], axis=-1)


def ld_dft_direct(x, sign=-1):
    """The O(N^2) definition (the check of ld_fft)."""
    x = np.asarray(x, CLD)
    n = x.shape[-1]
    k = np.arange(n, dtype=LD)
    # exponents reduced mod n exactly (integers) before the angle is formed
    w = np.exp(CLD(1j) * (LD(sign) * 2 * LD_PI * (np.outer(k, k) % n) / LD(n)))
    return x @ w


def ld_pa(kind, x, sat=0.0, p=0.0, toi=0.0):
    """oracle/refmath.py soft_limiter / rapp / toi in long double."""
    x = np.asarray(x, CLD)
    pw = x.real * x.real + x.imag * x.imag
    if kind == PA_NONE:
        return x.copy()
    if kind == PA_SOFTLIM:
        sc = np.where(pw <= LD(sat), LD(1), np.sqrt(LD(sat) / np.where(pw != 0, pw, LD(1))))
        return x * sc
    if kind == PA_RAPP:
        u = pw / LD(sat)  # (|x| / sqrt(sat))^(2 p) = (|x|^2 / sat)^p
        return x / np.power(LD(1) + np.power(u, LD(p)), LD(1) / (2 * LD(p)))
    if kind == PA_TOI:
        return x * (LD(1) - LD(toi) * pw)
    raise ValueError(kind)


def ld_chain(X, kind, sat=0.0, p=0.0, toi=0.0):
    """The kernel's IFFT -> PA -> FFT, both transforms un-normalised, in long double."""
    return ld_fft(ld_pa(kind, ld_fft(X, +1), sat, p, toi), -1)


def np_chain(X, kind, sat=0.0, p=0.0, toi=0.0):
    """The same chain by NumPy in X's own precision (np.fft keeps complex64 / complex128):
    the yardstick whose error against the long-double reference scales the bounds."""
    from oracle import refmath as rm
    X = np.asarray(X)
    rt = X.real.dtype.type
    n = X.shape[-1]
    x = np.fft.ifft(X, axis=-1) * rt(n)
    assert x.dtype == X.dtype
    if kind == PA_SOFTLIM:
        x = rm.soft_limiter(rt(sat), x)
    elif kind == PA_RAPP:
        x = rm.rapp(rt(sat), rt(p), x)
    elif kind == PA_TOI:
        x = rm.toi(rt(toi), x)
    x = np.asarray(x, X.dtype)
    y = np.fft.fft(x, axis=-1)
    assert y.dtype == X.dtype
    return y


def errors(got, ref):
    """Per row: (relative l2 = ||got - ref|| / ||ref||, max-abs = max |got - ref| / rms(ref)),
    formed in long double."""
    got, ref = np.asarray(got, CLD), np.asarray(ref, CLD)
    d = np.abs(got - ref)
    r2 = np.sum(np.abs(ref) ** 2, axis=-1)
    l2 = np.sqrt(np.sum(d * d, axis=-1) / r2)
    mx = np.max(d, axis=-1) / np.sqrt(r2 / ref.shape[-1])
    return np.asarray(l2, np.float64), np.asarray(mx, np.float64)


def ulp_err(got, ref, dtype=np.float64):
    """|got - ref| in units of the spacing of `dtype` at |ref| (ref: long double)."""
    ref = np.asarray(ref, LD)
    sp = np.spacing(np.abs(ref).astype(dtype)).astype(LD)
    return np.asarray(np.abs(np.asarray(got, LD) - ref) / sp, np.float64)


# ---------------------------------------------------------------- stage plan (csrc/team_fft.h)
def ilog2(n):
    return int(n).bit_length() - 1


def fft_nst(F, P):
    return (ilog2(F) + ilog2(P) - 1) // ilog2(P)


def fft_bits(F, P, s):
    if fft_nst(F, P) > 1:
        n, rest = fft_nst(F, P) - 1, ilog2(F) - ilog2(P)
        return ilog2(P) if s == n else rest // n + (1 if s < rest % n else 0)
    return ilog2(F)


def fft_bits_before(F, P, s):
    return sum(fft_bits(F, P, i) for i in range(s))


def stage_exponents(F, P):
    """Per entry of the stage twiddle table of an F-point, P-per-thread transform: the exponent
    e of exp(-j 2 pi e / F) (stages 1 .. NST - 1, [R][NS] blocks in order)."""
    out = []
    for st in range(1, fft_nst(F, P)):
        NS, R = 1 << fft_bits_before(F, P, st), 1 << fft_bits(F, P, st)
        for r in range(R):
            out += [jm * r * (F // (NS * R)) for jm in range(NS)]
    return np.array(out, np.int64)


def ct_rev(R, ns, jm, q):
    """team_fft.h ct_rev: the rows of a radix-R stage's cot-tan constants, in revolutions, as an
    exact fraction (numerator, denominator)."""
    d = R * ns
    if R == 8:
        num, den = [(-4 * jm, d), (-2 * jm, d), (-jm, d), (-8 * jm - d, 8 * d)][q]
    else:
        num, den = [(-8 * jm, d), (-4 * jm, d), (-2 * jm, d), (-16 * jm - d, 8 * d), (-jm, d), (-16 * jm - d, 16 * d),
                    (-8 * jm - d, 8 * d), (-16 * jm - 3 * d, 16 * d)][q]
    return num, den


def ct_angles(F, P):
    """Per entry of a transform's cot-tan region: the angle in revolutions as (num, den)."""
    out = []
    for st in range(1, fft_nst(F, P)):
        NS, R = 1 << fft_bits_before(F, P, st), 1 << fft_bits(F, P, st)
        for q in range(4 if R == 8 else 8):
            out += [ct_rev(R, NS, jm, q) for jm in range(NS)]
    return out


def ld_cis_rev(num, den):
    """exp(j 2 pi num / den) in long double, the fraction reduced to [0, 1) in integers first."""
    num = np.asarray(num, np.int64) % np.asarray(den, np.int64)
    a = 2 * LD_PI * num.astype(LD) / np.asarray(den).astype(LD)
    return np.cos(a) + CLD(1j) * np.sin(a)
