"""ctypes binding of libmimo_engine.so (include/mimo_engine.h).

This is the reference-side FFI a maintainer would add: plain pointers and sizes, no
torch types.  The library is built in-tree by ``__graft_entry__.build()`` (``make`` in
``csrc/``); there is no CPU fallback -- if the library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIMO_LIB") or os.path.join(_HERE, "libmimo_engine.so")

PA_KINDS = {"none": 0, "softlim": 1, "rapp": 2, "toi": 3}
CH_KINDS = {"rayleigh": 1, "los": 2, "two_path": 3, "table": 4, "tdl": 5}
RX_KINDS = {"cnc": 1, "mcnc": 2}
# Arithmetic type of the fused kernel: "f64" is the reference's own precision (complex128 /
# float64, the default); "f32" is the fast variant.  MIMO_PRECISION overrides the default.
PRECISIONS = {"f64": 0, "f32": 1}


def default_precision():
    p = os.environ.get("MIMO_PRECISION", "f64").lower()
    if p not in PRECISIONS:
        raise ValueError(f"MIMO_PRECISION must be one of {sorted(PRECISIONS)}")
    return p

_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_i8p = ctypes.POINTER(ctypes.c_int8)
_i16p = ctypes.POINTER(ctypes.c_int16)


class MimoConfig(ctypes.Structure):
    _fields_ = [("n_ant", ctypes.c_int32), ("n_sub_carr", ctypes.c_int32), ("n_fft", ctypes.c_int32),
                ("constel_size", ctypes.c_int32), ("cp_len", ctypes.c_int32), ("channel_kind", ctypes.c_int32),
                ("receiver_kind", ctypes.c_int32), ("device", ctypes.c_int32), ("rx_pos", ctypes.c_double * 3),
                ("rx_loc_var", ctypes.c_double), ("reroll_chan", ctypes.c_int32), ("precision", ctypes.c_int32),
                ("tx_pos", _dp), ("carrier_freqs", _dp), ("chan_table", _dp), ("chan_replay_period", ctypes.c_int32),
                ("csi_seed", ctypes.c_uint64)]


class MimoPoint(ctypes.Structure):
    _fields_ = [("ibo_db", ctypes.c_double), ("snr_db", ctypes.c_double), ("avg_symbol_power", ctypes.c_double),
                ("pa_kind", ctypes.c_int32), ("cnc_pa_kind", ctypes.c_int32), ("sat_pow", ctypes.c_double),
                ("p_hardness", ctypes.c_double), ("toi_coeff", ctypes.c_double), ("cnc_sat_pow", ctypes.c_double),
                ("cnc_toi_coeff", ctypes.c_double), ("cnc_alpha", ctypes.c_double), ("csi_eps", ctypes.c_double),
                ("array_alpha", ctypes.c_double)]


class LdpcCode(ctypes.Structure):
    """mimo_ldpc_code: a QC-LDPC code by its base matrix.  ``LdpcCode(z, table, n_dec_iters)`` with
    ``table`` [n_rows, n_cols] of shifts, -1 for a zero block: check i of base row r touches bit
    ``c z + (i + s) mod z`` of base column c.  ``table`` (int16, read-only) stays with the object."""
    _fields_ = [("z", ctypes.c_int32), ("n_rows", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("shifts", _i16p),
                ("n_dec_iters", ctypes.c_int32)]

    def __init__(self, z, table, n_dec_iters=10):
        t = np.asarray(table)
        if t.ndim != 2:
            raise ValueError("the shift table must be [n_rows, n_cols]")
        if t.size and (t.min() < -32768 or t.max() > 32767):  # (the rules are the library's to check)
            raise ValueError("shifts must fit int16")
        self.table = np.ascontiguousarray(t, dtype=np.int16)
        self.table.setflags(write=False)
        super().__init__(z=int(z), n_rows=t.shape[0], n_cols=t.shape[1], shifts=self.table.ctypes.data_as(_i16p),
                         n_dec_iters=int(n_dec_iters))

    @property
    def n_bits(self):
        """N = n_cols z code bits."""
        return self.n_cols * self.z

    def with_iters(self, n_dec_iters):
        return LdpcCode(self.z, self.table, n_dec_iters)


class TdlProfile(ctypes.Structure):
    """mimo_tdl: a power-delay profile.  ``TdlProfile(delays, powers, ant_amp=None)``: whole-sample
    delays (strictly ascending), linear powers (used as given) and, optionally, one amplitude per
    antenna (None: 1).  The arrays stay with the object; the rules are the library's to check."""
    _fields_ = [("n_taps", ctypes.c_int32), ("delays", _i32p), ("powers", _dp), ("ant_amp", _dp)]

    def __init__(self, delays, powers, ant_amp=None):
        d = np.asarray(delays)
        if d.ndim != 1 or np.asarray(powers).shape != d.shape:
            raise ValueError("delays and powers must be one-dimensional and of equal length")
        if d.size and (np.any(d != np.floor(d)) or d.min() < -2 ** 31 or d.max() >= 2 ** 31):
            raise ValueError("delays must be whole samples that fit int32")
        self.delays_arr = np.ascontiguousarray(d, dtype=np.int32)
        self.powers_arr = np.ascontiguousarray(powers, dtype=np.float64)
        self.amp_arr = None if ant_amp is None else np.ascontiguousarray(ant_amp, dtype=np.float64).reshape(-1)
        super().__init__(n_taps=int(d.size), delays=self.delays_arr.ctypes.data_as(_i32p),
                         powers=self.powers_arr.ctypes.data_as(_dp),
                         ant_amp=self.amp_arr.ctypes.data_as(_dp) if self.amp_arr is not None else None)


class RayProfile(ctypes.Structure):
    """mimo_rays: a ray-cluster profile.  ``RayProfile(delays, ray_tap, ray_amp, steer, ray_kind=None)``:
    whole-sample tap ``delays``, the tap of every ray (non-decreasing from 0 in steps of 0 or 1),
    the rays' amplitudes, their steering vectors ``steer`` [n_ant, R] complex and, optionally, their
    kinds (0 diffuse, 1 specular; None: all diffuse).  The arrays stay with the object; the rules are
    the library's to check."""
    _fields_ = [("n_taps", ctypes.c_int32), ("delays", _i32p), ("n_rays", ctypes.c_int32), ("ray_tap", _i32p),
                ("ray_amp", _dp), ("ray_kind", ctypes.POINTER(ctypes.c_uint8)), ("steer", _dp)]

    def __init__(self, delays, ray_tap, ray_amp, steer, ray_kind=None):
        d, rt = np.asarray(delays), np.asarray(ray_tap)
        if d.ndim != 1 or rt.ndim != 1:
            raise ValueError("delays and ray_tap must be one-dimensional")
        for name, v in (("delays", d), ("ray_tap", rt)):
            if v.size and (np.any(v != np.floor(v)) or v.min() < -2 ** 31 or v.max() >= 2 ** 31):
                raise ValueError(f"{name} must be whole numbers that fit int32")
        if np.asarray(ray_amp).shape != rt.shape:
            raise ValueError("ray_amp must hold one amplitude per ray")
        st = np.asarray(steer)
        if st.ndim != 2 or st.shape[1] != rt.size:
            raise ValueError("steer must be [n_ant, n_rays]")
        self.n_ant = st.shape[0]
        self.delays_arr = np.ascontiguousarray(d, dtype=np.int32)
        self.tap_arr = np.ascontiguousarray(rt, dtype=np.int32)
        self.amp_arr = np.ascontiguousarray(ray_amp, dtype=np.float64)
        self.steer_arr = np.ascontiguousarray(st, dtype=np.complex128).view(np.float64)
        self.kind_arr = None
        if ray_kind is not None:
            k = np.asarray(ray_kind)
            if k.shape != rt.shape:
                raise ValueError("ray_kind must hold one kind per ray")
            if k.size and (np.any(k != np.floor(k)) or k.min() < 0 or k.max() > 255):
                raise ValueError("ray_kind must be 0 (diffuse) or 1 (specular)")
            self.kind_arr = np.ascontiguousarray(k, dtype=np.uint8)
        super().__init__(n_taps=int(d.size), delays=self.delays_arr.ctypes.data_as(_i32p), n_rays=int(rt.size),
                         ray_tap=self.tap_arr.ctypes.data_as(_i32p), ray_amp=self.amp_arr.ctypes.data_as(_dp),
                         ray_kind=(self.kind_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
                                   if self.kind_arr is not None else None),
                         steer=self.steer_arr.ctypes.data_as(_dp))


SYMBOLS = {
    "mimo_abi_version": (ctypes.c_int32, []),
    "mimo_last_error": (ctypes.c_char_p, []),
    "mimo_device_count": (ctypes.c_int32, []),
    "mimo_engine_create": (ctypes.c_void_p, [ctypes.POINTER(MimoConfig)]),
    "mimo_engine_set_point": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(MimoPoint)]),
    "mimo_engine_run": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _i32p,
                                         ctypes.c_int32, ctypes.c_int32, _u64p, _u64p, _u32p]),
    "mimo_engine_run_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                _u32p]),
    "mimo_measure_width": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
    "mimo_engine_measure_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                    _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                    _u32p, _dp, _dp]),
    "mimo_spectrum_width": (ctypes.c_int32, [ctypes.c_int32]),
    "mimo_engine_spectrum_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                     _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                     _u32p, _dp, _dp]),
    "mimo_beam_width": (ctypes.c_int32, [ctypes.c_int32]),
    "mimo_engine_beam_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                 _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                 _u32p, _dp, ctypes.c_int32, _dp, _dp]),
    "mimo_envelope_width": (ctypes.c_int32, []),
    "mimo_envelope_edges": (ctypes.c_int32, [_dp]),
    "mimo_engine_envelope_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                     _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                     _u32p, ctypes.c_double, _dp, _dp]),
    "mimo_soft_width": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
    "mimo_engine_soft_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                 _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                 _u32p, ctypes.c_double, _dp, _dp]),
    "mimo_coded_width": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]),
    "mimo_coded_codewords": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(LdpcCode)]),
    "mimo_engine_coded_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                  _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                  _u32p, ctypes.POINTER(LdpcCode), ctypes.c_double, _dp, _dp, _i8p]),
    "mimo_turbo_width": (ctypes.c_int32, [ctypes.c_int32]),
    "mimo_engine_turbo_points": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(MimoPoint), _u64p,
                                                  _u64p, _u64p, _i32p, ctypes.c_int32, ctypes.c_int32, _u64p, _u64p,
                                                  _u32p, ctypes.POINTER(LdpcCode), ctypes.c_double, ctypes.c_int32, _dp,
                                                  _dp, _i8p, _dp]),
    "mimo_engine_cnc_step": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(MimoPoint), _dp, _i32p, ctypes.c_int64,
                                              _dp]),
    "mimo_engine_last_decode_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "mimo_bank_capacity": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "mimo_engine_set_channel_bank": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32, _dp]),
    "mimo_engine_set_tdl": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(TdlProfile)]),
    "mimo_tdl_channels": (ctypes.c_int32, [ctypes.POINTER(TdlProfile), ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                           ctypes.c_uint64, ctypes.c_int64, _dp, _dp]),
    "mimo_engine_set_rays": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(RayProfile)]),
    "mimo_rays_channels": (ctypes.c_int32, [ctypes.POINTER(RayProfile), ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_int64, _dp, _dp, _dp]),
    "mimo_engine_last_chan_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "mimo_ldpc_decode": (ctypes.c_int32, [ctypes.POINTER(LdpcCode), _i8p, ctypes.c_int64, _i16p]),
    "mimo_engine_last_kernel_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "mimo_engine_last_beam_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "mimo_engine_describe": (ctypes.c_char_p, [ctypes.c_void_p]),
    "mimo_engine_destroy": (None, [ctypes.c_void_p]),
    "mimo_qam_map": (ctypes.c_int32, [ctypes.c_int32, _i32p, ctypes.c_int64, _dp]),
    "mimo_qam_slice": (ctypes.c_int32, [ctypes.c_int32, _dp, ctypes.c_int64, _i32p]),
    "mimo_qam_llr": (ctypes.c_int32, [ctypes.c_int32, _dp, ctypes.c_int64, _dp, _dp]),
    "mimo_qam_softbits": (ctypes.c_int32, [ctypes.c_int32, _dp, ctypes.c_int64, _dp]),
    "mimo_fft": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, _dp, _dp]),
    "mimo_ofdm_tx": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _dp, _dp]),
    "mimo_ofdm_rx": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _dp, _dp]),
    "mimo_pa": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, _dp,
                                 ctypes.c_int64, _dp]),
    "mimo_calc_alpha": (ctypes.c_int32, [_dp, ctypes.c_int64, _dp]),
    "mimo_mrt_precode": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, _dp, _dp]),
    "mimo_combine": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, _dp, _dp, _dp]),
    "mimo_awgn": (ctypes.c_int32, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_double, _dp, _dp]),
    "mimo_count_bit_errors": (ctypes.c_int32, [_i64p, _i64p, ctypes.c_int64, _i64p]),
    "mimo_cnc_receive": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _i32p,
                                          ctypes.c_int32, _dp, _i32p]),
    "mimo_cnc_receive_ex": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _i32p,
                                             ctypes.c_int32, _dp, _i32p, _dp]),
}

_lib = None


class EngineError(RuntimeError):
    pass


ABI_VERSION = 8  # include/mimo_engine.h MIMO_ABI_VERSION
MEAS_FIXED = 5   # include/mimo_engine.h MIMO_MEAS_FIXED
SPEC_FIXED = 3   # include/mimo_engine.h MIMO_SPEC_FIXED
BEAM_FIXED = 5   # include/mimo_engine.h MIMO_BEAM_FIXED
ENV_BINS = 128   # include/mimo_engine.h MIMO_ENV_BINS
ENV_FIXED = 4    # include/mimo_engine.h MIMO_ENV_FIXED
ENV_WIDTH = 2 * ENV_BINS + ENV_FIXED
SOFT_BINS = 256  # include/mimo_engine.h MIMO_SOFT_BINS
CODED_FIXED = 4  # include/mimo_engine.h MIMO_CODED_FIXED
TURBO_MAX_PASSES = 16  # include/mimo_engine.h MIMO_TURBO_MAX_PASSES
TDL_MAX_TAPS = 64  # include/mimo_engine.h MIMO_TDL_MAX_TAPS
RAYS_MAX = 1024    # include/mimo_engine.h MIMO_RAYS_MAX


def lib():
    """Load the HIP engine library; raises if it was not built (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"{LIB_PATH} not found: build it with __graft_entry__.build() (make -C csrc)")
        handle = ctypes.CDLL(LIB_PATH)
        # the ABI first: the structures below are ABI 8's (mimo_point.array_alpha),
        # and a stale library lacks the newer entry points -- binding them first would raise a
        # bare AttributeError instead of this message
        ver = getattr(handle, "mimo_abi_version", None)
        if ver is None:
            raise EngineError(f"{LIB_PATH} exports no mimo_abi_version (older than ABI 2): rebuild it")
        ver.restype, ver.argtypes = ctypes.c_int32, []
        if ver() != ABI_VERSION:
            raise EngineError(f"{LIB_PATH} is ABI {ver()}, this module ABI {ABI_VERSION}: rebuild it")
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name, None)
            if fn is None:
                raise EngineError(f"{LIB_PATH} (ABI {ABI_VERSION}) lacks {name}: rebuild it")
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def _check(rc):
    if rc != 0:
        raise EngineError(lib().mimo_last_error().decode() or f"mimo error {rc}")


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def as_iq(x):
    """complex array -> contiguous float64 (re, im) view."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128))
    return x.view(np.float64)


def _ratio_db(num, den):
    """10 log10(num / den) elementwise; a zero denominator gives inf (no warning, no NaN)."""
    num = np.asarray(num, np.float64)
    den = np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.inf)
    ok = (den > 0) & (num > 0)
    np.divide(num, den, out=out, where=ok)
    np.log10(out, out=out, where=ok)
    np.multiply(out, 10.0, out=out, where=ok)
    out[np.broadcast_to((num <= 0) & (den > 0), out.shape)] = -np.inf
    return out if out.ndim else float(out)


class SignalStats:
    """Signal / distortion powers of a measure call (mimo_engine_measure_points): one row
    ``[Es, Ez0, Re C, Im C, Ed0, Ee_0 ...]`` of sums over trials and data sub-carriers, with the
    bit-error totals of the same trials.  ``a + b`` pools two measurements (sums add)."""

    def __init__(self, row, err=None, bits=None):
        self.row = np.array(row, np.float64).reshape(-1)
        if self.row.size < MEAS_FIXED + 1:
            raise ValueError(f"a measure row has at least {MEAS_FIXED + 1} entries")
        n_idx = self.row.size - MEAS_FIXED
        self.err = np.zeros(n_idx, np.uint64) if err is None else np.array(err, np.uint64).reshape(-1)
        self.bits = np.zeros(n_idx, np.uint64) if bits is None else np.array(bits, np.uint64).reshape(-1)
        if self.err.size != n_idx or self.bits.size != n_idx:
            raise ValueError("err and bits must have one entry per counter index of the row")

    @classmethod
    def from_totals(cls, es, ez0, c, ed0, ee, err=None, bits=None):
        c = complex(c)
        return cls(np.concatenate([[es, ez0, c.real, c.imag, ed0], np.atleast_1d(np.asarray(ee, np.float64))]),
                   err, bits)

    es = property(lambda self: float(self.row[0]))
    ez0 = property(lambda self: float(self.row[1]))
    c = property(lambda self: complex(self.row[2], self.row[3]))
    ed0 = property(lambda self: float(self.row[4]))
    ee = property(lambda self: self.row[MEAS_FIXED:].copy())

    @property
    def gain(self):
        """beta = C / Es: the least-squares (Bussgang) gain of the noiseless received signal."""
        return self.c / self.es if self.es > 0 else complex(np.inf)

    @property
    def sdr_db(self):
        """|C|^2 / (Es Ez0 - |C|^2): signal power over the power uncorrelated with it."""
        c2 = abs(self.c) ** 2
        return _ratio_db(c2, self.es * self.ez0 - c2)

    @property
    def slicer_sdr_db(self):
        """Es / Ed0: what the fixed AGC leaves at the slicer, without noise."""
        return _ratio_db(self.es, self.ed0)

    @property
    def sndr_db(self):
        """Es / Ee_i per counter index: noise plus residual distortion at the slicer."""
        return _ratio_db(self.es, self.row[MEAS_FIXED:])

    @property
    def ber(self):
        out = np.zeros(self.err.size)
        np.divide(self.err.astype(np.float64), self.bits.astype(np.float64), out=out, where=self.bits > 0)
        return out

    def __add__(self, other):
        if not isinstance(other, SignalStats):
            return NotImplemented
        if other.row.size != self.row.size:
            raise ValueError("measurements with different counter layouts cannot be pooled")
        return SignalStats(self.row + other.row, self.err + other.err, self.bits + other.bits)

    def __repr__(self):
        return (f"SignalStats(sdr_db={self.sdr_db:.3f}, slicer_sdr_db={self.slicer_sdr_db:.3f}, "
                f"sndr_db={np.array2string(self.sndr_db, precision=3)})")


def inband_bins(n_fft, n_sub_carr):
    """Data sub-carrier k -> FFT bin (modulation.py:266-267, 293): the negative half first, DC skipped."""
    half = n_sub_carr // 2
    return np.concatenate((np.arange(n_fft - half, n_fft), np.arange(1, half + 1)))


class SpectrumStats:
    """Radiated spectrum of a spectrum call (mimo_engine_spectrum_points): one row
    ``[psd[0] ... psd[F-1], Ex, Re C, Im C]`` of sums over trials and antennas -- the power the
    array radiates per FFT bin (numpy.fft order), its precoded input power and the correlation of
    output and input over the ``n_sub_carr`` data sub-carriers.  ``a + b`` pools two measurements."""

    def __init__(self, row, n_sub_carr, n_trials=None):
        self.row = np.array(row, np.float64).reshape(-1)
        self.n_fft = self.row.size - SPEC_FIXED
        self.n_sub_carr = int(n_sub_carr)
        if self.n_fft < 4 or not 0 < self.n_sub_carr <= self.n_fft - 2 or self.n_sub_carr % 2:
            raise ValueError("a spectrum row has n_fft + 3 entries, and n_sub_carr is even and at most n_fft - 2")
        self.n_trials = None if n_trials is None else int(n_trials)

    psd = property(lambda self: self.row[:self.n_fft].copy())
    ex = property(lambda self: float(self.row[self.n_fft]))
    c = property(lambda self: complex(self.row[self.n_fft + 1], self.row[self.n_fft + 2]))

    @property
    def freq_index(self):
        """Signed bin index of ``psd_centered``'s entries: -F/2 ... F/2 - 1."""
        return np.arange(-(self.n_fft // 2), self.n_fft - self.n_fft // 2)

    @property
    def psd_centered(self):
        """``psd`` fft-shifted: most negative frequency first, DC in the middle (see ``freq_index``)."""
        return np.fft.fftshift(self.row[:self.n_fft])

    @property
    def total(self):
        return float(self.row[:self.n_fft].sum())

    @property
    def inband(self):
        """Power in the data sub-carriers' bins (the DC bin is out of band)."""
        return float(self.row[inband_bins(self.n_fft, self.n_sub_carr)].sum())

    @property
    def oob(self):
        mask = np.ones(self.n_fft, bool)
        mask[inband_bins(self.n_fft, self.n_sub_carr)] = False
        return float(self.row[:self.n_fft][mask].sum())

    @property
    def oob_ratio_db(self):
        """10 log10(oob / total); -inf without out-of-band power."""
        return _ratio_db(self.oob, self.total)

    @property
    def gain(self):
        """C / Ex: the array's measured Bussgang gain."""
        return self.c / self.ex if self.ex > 0 else complex(np.inf)

    @property
    def efficiency(self):
        """total / Ex: radiated power over precoded input power."""
        return self.total / self.ex if self.ex > 0 else np.inf

    @property
    def radiated_sdr_db(self):
        """|C|^2 / Ex over inband - |C|^2 / Ex: in-band power correlated with the input over the rest."""
        sig = abs(self.c) ** 2 / self.ex if self.ex > 0 else np.inf
        return _ratio_db(sig, self.inband - sig)

    @property
    def psd_rel_db(self):
        """``psd`` over the mean in-band ``psd``, in dB."""
        return _ratio_db(self.row[:self.n_fft], self.inband / self.n_sub_carr)

    def __add__(self, other):
        if not isinstance(other, SpectrumStats):
            return NotImplemented
        if other.row.size != self.row.size or other.n_sub_carr != self.n_sub_carr:
            raise ValueError("spectra of different systems cannot be pooled")
        n = None if self.n_trials is None or other.n_trials is None else self.n_trials + other.n_trials
        return SpectrumStats(self.row + other.row, self.n_sub_carr, n)

    def __repr__(self):
        return (f"SpectrumStats(n_fft={self.n_fft}, oob_ratio_db={self.oob_ratio_db:.3f}, "
                f"radiated_sdr_db={self.radiated_sdr_db:.3f}, gain={abs(self.gain):.4f}, "
                f"efficiency={self.efficiency:.4f})")


class BeamStats:
    """Beampattern of a beam call (mimo_engine_beam_points): per probe position the row
    ``[Py_in, Py_oob, Px, Re C, Im C]`` of sums over trials and FFT bins -- the in-band and the
    out-of-band power the array radiates towards the probe through a line-of-sight channel, the
    power its precoded input would deliver there, and their in-band correlation.  Every figure
    below is an array with one entry per probe.  ``a + b`` pools two measurements."""

    def __init__(self, rows, n_trials=None):
        self.rows = np.array(rows, np.float64)
        if self.rows.ndim != 2 or self.rows.shape[0] < 1 or self.rows.shape[1] != BEAM_FIXED:
            raise ValueError(f"beam rows are [n_probes, {BEAM_FIXED}]")
        self.n_trials = None if n_trials is None else int(n_trials)

    n_probes = property(lambda self: self.rows.shape[0])
    power_inband = property(lambda self: self.rows[:, 0].copy())
    power_oob = property(lambda self: self.rows[:, 1].copy())
    input_power = property(lambda self: self.rows[:, 2].copy())
    c = property(lambda self: self.rows[:, 3] + 1j * self.rows[:, 4])

    @property
    def gain(self):
        """C / Px: the array's Bussgang gain towards each probe (inf where no input power arrives)."""
        out = np.full(self.n_probes, complex(np.inf))
        np.divide(self.c, self.rows[:, 2], out=out, where=self.rows[:, 2] > 0)
        return out

    @property
    def signal(self):
        """|C|^2 / Px: the in-band power correlated with the precoded input."""
        out = np.full(self.n_probes, np.inf)
        np.divide(self.rows[:, 3] ** 2 + self.rows[:, 4] ** 2, self.rows[:, 2], out=out, where=self.rows[:, 2] > 0)
        return out

    @property
    def distortion(self):
        """Py_in - |C|^2 / Px: the in-band power uncorrelated with the input."""
        return self.rows[:, 0] - self.signal

    @property
    def sdr_db(self):
        """signal over distortion, in dB; inf where rounding leaves no distortion."""
        return _ratio_db(self.signal, self.distortion)

    _PATTERNS = ("signal", "distortion", "power_oob", "power_inband", "input_power")

    def _pattern(self, which):
        if which not in self._PATTERNS:
            raise ValueError("which must be signal, distortion, power_oob, power_inband or input_power")
        return getattr(self, which)

    def directivity(self, which="signal"):
        """max / mean over the probes of ``signal``, ``distortion``, ``power_oob``, ``power_inband`` or
        ``input_power``."""
        v = self._pattern(which)
        return float(v.max() / v.mean())

    def pattern_db(self, which="signal", ref=None):
        """The pattern ``which`` (as for ``directivity``) over ``ref`` in dB, per probe; ``ref``
        defaults to the mean ``signal`` over the probes.  -inf where nothing is radiated."""
        return _ratio_db(self._pattern(which), float(np.mean(self.signal)) if ref is None else ref)

    def __add__(self, other):
        if not isinstance(other, BeamStats):
            return NotImplemented
        if other.rows.shape != self.rows.shape:
            raise ValueError("beampatterns over different probe lists cannot be pooled")
        n = None if self.n_trials is None or other.n_trials is None else self.n_trials + other.n_trials
        return BeamStats(self.rows + other.rows, n)

    def __repr__(self):
        return (f"BeamStats(n_probes={self.n_probes}, signal directivity={self.directivity('signal'):.3f}, "
                f"distortion directivity={self.directivity('distortion'):.3f})")


def envelope_edges():
    """Lower edges of the envelope bins 1 ... 127 in units of u = |.|^2 / ref_pow (mimo_envelope_edges)."""
    out = np.empty(ENV_BINS - 1, np.float64)
    _check(lib().mimo_envelope_edges(_ptr(out, ctypes.c_double)))
    return out


class EnvelopeStats:
    """Envelope of an envelope call (mimo_engine_envelope_points): one row
    ``[hist_in[0..127], hist_out[0..127], Pin, Pout, Re C, Im C]`` of sums over trials, antennas and
    time samples -- the histograms of the instantaneous power at the PA inputs and outputs over the
    bins whose lower edges are ``edges`` (in units of ``u = |.|^2 / ref_pow``; bin 0 takes everything
    below ``edges[0]``), the two total powers and the correlation of output and input.
    ``a + b`` pools two measurements of one system taken with the same ``ref_pow``."""

    def __init__(self, row, n_ant, n_fft, n_trials, ref_pow):
        self.row = np.array(row, np.float64).reshape(-1)
        if self.row.size != ENV_WIDTH:
            raise ValueError(f"an envelope row has {ENV_WIDTH} entries")
        self.n_ant, self.n_fft, self.n_trials = int(n_ant), int(n_fft), int(n_trials)
        self.ref_pow = float(ref_pow)
        if self.n_ant < 1 or self.n_fft < 1 or self.n_trials < 0 or not self.ref_pow > 0:
            raise ValueError("n_ant and n_fft are >= 1, n_trials >= 0 and ref_pow > 0")
        self.edges = envelope_edges()

    hist_in = property(lambda self: self.row[:ENV_BINS].copy())
    hist_out = property(lambda self: self.row[ENV_BINS:2 * ENV_BINS].copy())
    p_in = property(lambda self: float(self.row[2 * ENV_BINS]))
    p_out = property(lambda self: float(self.row[2 * ENV_BINS + 1]))
    c = property(lambda self: complex(self.row[2 * ENV_BINS + 2], self.row[2 * ENV_BINS + 3]))

    @property
    def edges_db(self):
        return 10.0 * np.log10(self.edges)

    @property
    def n_samples(self):
        """Samples per histogram: trials x antennas x n_fft."""
        return self.n_trials * self.n_ant * self.n_fft

    def _ccdf(self, hist):
        # exact tail sums: the cells are integers, their sums stay below 2^53
        tail = np.cumsum(hist[::-1])[::-1][1:]
        out = np.zeros(ENV_BINS - 1)
        if self.n_samples > 0:
            out = tail / float(self.n_samples)
        return out

    @property
    def ccdf_in(self):
        """P(u >= edges[i]) at the PA inputs."""
        return self._ccdf(self.row[:ENV_BINS])

    @property
    def ccdf_out(self):
        """P(u >= edges[i]) at the PA outputs."""
        return self._ccdf(self.row[ENV_BINS:2 * ENV_BINS])

    @property
    def mean_in_db(self):
        """Mean input sample power over ref_pow, in dB."""
        return _ratio_db(self.p_in, self.n_samples * self.ref_pow)

    @property
    def efficiency(self):
        """Pout / Pin: radiated power over PA input power."""
        return self.p_out / self.p_in if self.p_in > 0 else np.inf

    @property
    def gain(self):
        """C / Pin: the array's measured Bussgang gain."""
        return self.c / self.p_in if self.p_in > 0 else complex(np.inf)

    def level_db(self, prob, which="in"):
        """The smallest edge [dB] whose CCDF is <= ``prob`` (``which``: "in" or "out"); nan if none."""
        if which not in ("in", "out"):
            raise ValueError('which must be "in" or "out"')
        ccdf = self.ccdf_in if which == "in" else self.ccdf_out
        ok = np.flatnonzero(ccdf <= prob)
        return float(self.edges_db[ok[0]]) if ok.size else float("nan")

    def __add__(self, other):
        if not isinstance(other, EnvelopeStats):
            return NotImplemented
        if (other.n_ant, other.n_fft, other.ref_pow) != (self.n_ant, self.n_fft, self.ref_pow):
            raise ValueError("envelopes of different systems or reference powers cannot be pooled")
        return EnvelopeStats(self.row + other.row, self.n_ant, self.n_fft, self.n_trials + other.n_trials, self.ref_pow)

    def __repr__(self):
        return (f"EnvelopeStats(n_samples={self.n_samples}, mean_in_db={self.mean_in_db:.3f}, "
                f"level_db(1e-3)={self.level_db(1e-3):.2f}, efficiency={self.efficiency:.4f}, "
                f"gain={abs(self.gain):.4f})")


class SoftStats:
    """Bit reliabilities of a soft call (mimo_engine_soft_points): ``hist[n_idx][256]``, per counter
    index ([clean] + one per recorded iteration) the number of bit reliabilities
    ``rho = +-lambda`` (the max-log soft bit signed by the transmitted bit; ``rho < 0`` is a
    hard-decision error) in each of 256 linear bins of width ``rho_max / 128``; bin 128 opens at 0,
    bins 0 and 255 take everything beyond ``-+rho_max``.  From it the bit-wise mutual information of
    the demapper's outputs, the BICM generalised mutual information (GMI), which predicts what a
    coded link gets from the same trials: with the decoder's LLR ``scale * rho``,
    ``gmi(scale) = 1 - mean log2(1 + exp(-scale rho))``, evaluated on the bin midpoints.
    ``a + b`` (``a.pool(b)``) pools two measurements of one system taken with the same ``rho_max``."""

    def __init__(self, hist, rho_max, constel_size, n_trials):
        self.hist = np.array(hist, np.float64).reshape(-1, SOFT_BINS)
        self.rho_max, self.constel_size, self.n_trials = float(rho_max), int(constel_size), int(n_trials)
        if not (self.rho_max > 0 and np.isfinite(self.rho_max)) or self.constel_size < 4 or self.n_trials < 0:
            raise ValueError("rho_max is finite and > 0, constel_size >= 4 and n_trials >= 0")

    @property
    def n_idx(self):
        return self.hist.shape[0]

    @property
    def width(self):
        """The bin width rho_max / 128."""
        return self.rho_max / 128.0

    @property
    def centres(self):
        """The bin midpoints (bins 0 and 255 stand for everything beyond them)."""
        return (np.arange(SOFT_BINS) - 128 + 0.5) * self.width

    @property
    def n_bits(self):
        """Reliabilities per counter index (exact: the cells are integers below 2^53)."""
        return self.hist.sum(axis=1)

    def _share(self, cells):
        n = self.n_bits
        out = np.zeros(self.n_idx)
        np.divide(cells, n, out=out, where=n > 0)
        return out

    def ber(self):
        """The share of reliabilities below 0 (bins 0 ... 127): the hard-decision BER, per index."""
        return self._share(self.hist[:, :128].sum(axis=1))

    def clamped(self):
        """The share in bins 0 and 255, beyond the range: choose a larger rho_max if it matters."""
        return self._share(self.hist[:, 0] + self.hist[:, -1])

    def nominal_scale(self, noise_var):
        """4 / noise_var: the scale that turns rho into the max-log LLR of a Gaussian channel whose
        complex noise has variance ``noise_var`` in lattice units (``mimo_qam_llr``'s argument)."""
        return 4.0 / float(noise_var)

    def gmi(self, scale=None):
        """Per index, ``1 - sum_b h_b log2(1 + exp(-scale c_b)) / N`` in bits per coded bit (0 where
        nothing was measured); ``scale`` one number or one per index; None: the maximum over
        ``scale > 0`` (at ``best_scale()``)."""
        if scale is None:
            return self.gmi(self.best_scale())
        s = np.broadcast_to(np.asarray(scale, np.float64), (self.n_idx,))
        loss = (self.hist * np.logaddexp(0.0, -s[:, None] * self.centres[None, :])).sum(axis=1) / np.log(2.0)
        return np.where(self.n_bits > 0, 1.0 - self._share(loss), 0.0)

    def best_scale(self, iters=120):
        """Per index the scale that maximises ``gmi(scale)``: a golden-section search on
        ``log scale`` (the function is concave in ``scale``, so it has one maximum there too) between
        ``1e-3 / rho_max`` and ``2e3 / width``, where every LLR is negligible / saturated.  A histogram
        without errors keeps growing with the scale and returns the upper end."""
        lo = np.full(self.n_idx, np.log(1e-3 / self.rho_max))
        hi = np.full(self.n_idx, np.log(2e3 / self.width))
        g = (np.sqrt(5.0) - 1.0) / 2.0
        f = lambda t: self.gmi(np.exp(t))
        a, b = hi - g * (hi - lo), lo + g * (hi - lo)
        fa, fb = f(a), f(b)
        for _ in range(int(iters)):
            left = fa > fb   # the maximum lies in [lo, b]
            hi = np.where(left, b, hi)
            lo = np.where(left, lo, a)
            a, b = hi - g * (hi - lo), lo + g * (hi - lo)
            fa, fb = f(a), f(b)
        return np.exp(0.5 * (lo + hi))

    def rate(self):
        """``log2(constel_size) gmi()``: achievable bits per data sub-carrier, per index."""
        return np.log2(self.constel_size) * self.gmi()

    def pool(self, other):
        if not isinstance(other, SoftStats):
            return NotImplemented
        if (other.constel_size, other.rho_max, other.n_idx) != (self.constel_size, self.rho_max, self.n_idx):
            raise ValueError("reliabilities of different systems or ranges cannot be pooled")
        return SoftStats(self.hist + other.hist, self.rho_max, self.constel_size, self.n_trials + other.n_trials)

    __add__ = pool

    def __repr__(self):
        return (f"SoftStats(n_idx={self.n_idx}, n_trials={self.n_trials}, rho_max={self.rho_max:g}, "
                f"ber={np.array2string(self.ber(), precision=3)}, gmi={np.array2string(self.gmi(), precision=4)})")


class CodedStats:
    """Coded-link errors of a coded call (mimo_engine_coded_points): ``cells[n_idx][4]``, per counter
    index ([clean] + one per recorded iteration) over all decoded codewords the number of channel
    values below 0 (uncoded errors at the decoded positions), of wrong bits after the decoder, of
    wrong frames, and of frames whose hard decision fails a parity check.  ``n_frames`` codewords of
    ``n_code_bits`` bits each were decoded per index.  A frame the checks flag is no codeword and
    therefore wrong, so the flagged frames are among the wrong ones and ``undetected()`` =
    ``fer() - syndrome_rate()`` is the share of frames that converged to a wrong codeword.
    ``a + b`` (``a.pool(b)``) pools two measurements of one system and code."""

    def __init__(self, cells, n_frames, n_code_bits):
        self.cells = np.array(cells, np.float64).reshape(-1, CODED_FIXED)
        self.n_frames, self.n_code_bits = int(n_frames), int(n_code_bits)
        if self.n_frames < 0 or self.n_code_bits < 1:
            raise ValueError("n_frames >= 0 and n_code_bits >= 1")

    @property
    def n_idx(self):
        return self.cells.shape[0]

    @property
    def n_bits(self):
        """Decoded bits per counter index."""
        return self.n_frames * self.n_code_bits

    def _share(self, col, n):
        return self.cells[:, col] / n if n > 0 else np.zeros(self.n_idx)

    def raw_ber(self):
        """Uncoded BER at the decoded positions, per index."""
        return self._share(0, self.n_bits)

    def ber(self):
        """BER after the decoder, per index."""
        return self._share(1, self.n_bits)

    def fer(self):
        """Share of codewords with any wrong bit, per index."""
        return self._share(2, self.n_frames)

    def syndrome_rate(self):
        """Share of codewords whose hard decision is no codeword (a detected failure), per index."""
        return self._share(3, self.n_frames)

    def undetected(self):
        """Share of codewords that are wrong and pass every parity check, per index."""
        n = self.n_frames
        return (self.cells[:, 2] - self.cells[:, 3]) / n if n > 0 else np.zeros(self.n_idx)

    def pool(self, other):
        if not isinstance(other, CodedStats):
            return NotImplemented
        if (other.n_code_bits, other.n_idx) != (self.n_code_bits, self.n_idx):
            raise ValueError("coded errors of different codes or iteration lists cannot be pooled")
        return CodedStats(self.cells + other.cells, self.n_frames + other.n_frames, self.n_code_bits)

    __add__ = pool

    def __repr__(self):
        return (f"CodedStats(n_idx={self.n_idx}, n_frames={self.n_frames}, n_code_bits={self.n_code_bits}, "
                f"raw_ber={np.array2string(self.raw_ber(), precision=3)}, "
                f"ber={np.array2string(self.ber(), precision=3)}, fer={np.array2string(self.fer(), precision=3)})")


class TurboStats:
    """Coded-link errors of a turbo call (mimo_engine_turbo_points): ``cells[n_passes][4]``, per pass of
    the decoder-aided CNC receiver the four cells of ``CodedStats`` -- channel values below 0 at the
    decoded positions, wrong bits after the decoder, wrong frames, frames that fail a parity check --
    over ``n_frames`` codewords of ``n_code_bits`` bits each.  Pass 0 is the coded mode's CNC iteration
    0.  ``a + b`` (``a.pool(b)``) pools two measurements of one system, code and number of passes."""

    def __init__(self, cells, n_frames, n_code_bits):
        self.cells = np.array(cells, np.float64).reshape(-1, CODED_FIXED)
        self.n_frames, self.n_code_bits = int(n_frames), int(n_code_bits)
        if self.n_frames < 0 or self.n_code_bits < 1:
            raise ValueError("n_frames >= 0 and n_code_bits >= 1")
        if not 1 <= self.cells.shape[0] <= TURBO_MAX_PASSES:
            raise ValueError(f"n_passes must be in [1, {TURBO_MAX_PASSES}]")

    @property
    def n_passes(self):
        return self.cells.shape[0]

    @property
    def n_bits(self):
        """Decoded bits per pass."""
        return self.n_frames * self.n_code_bits

    def _share(self, col, n):
        return self.cells[:, col] / n if n > 0 else np.zeros(self.n_passes)

    def raw_ber(self):
        """Uncoded BER at the decoded positions, per pass."""
        return self._share(0, self.n_bits)

    def ber(self):
        """BER after the decoder, per pass."""
        return self._share(1, self.n_bits)

    def fer(self):
        """Share of codewords with any wrong bit, per pass."""
        return self._share(2, self.n_frames)

    def syndrome_rate(self):
        """Share of codewords whose hard decision is no codeword, per pass."""
        return self._share(3, self.n_frames)

    def undetected(self):
        """Share of codewords that are wrong and pass every parity check, per pass."""
        n = self.n_frames
        return (self.cells[:, 2] - self.cells[:, 3]) / n if n > 0 else np.zeros(self.n_passes)

    def pool(self, other):
        if not isinstance(other, TurboStats):
            return NotImplemented
        if (other.n_code_bits, other.n_passes) != (self.n_code_bits, self.n_passes):
            raise ValueError("turbo errors of different codes or numbers of passes cannot be pooled")
        return TurboStats(self.cells + other.cells, self.n_frames + other.n_frames, self.n_code_bits)

    __add__ = pool

    def __repr__(self):
        return (f"TurboStats(n_passes={self.n_passes}, n_frames={self.n_frames}, n_code_bits={self.n_code_bits}, "
                f"raw_ber={np.array2string(self.raw_ber(), precision=3)}, "
                f"ber={np.array2string(self.ber(), precision=3)}, fer={np.array2string(self.fer(), precision=3)})")


class Engine:
    """One configured system (the deep-copied objects of a ``Link``) on one GPU."""

    def __init__(self, n_ant, n_sub_carr, n_fft, constel_size, cp_len, channel, receiver, tx_pos, rx_pos,
                 rx_loc_var, carrier_freqs, reroll=True, device=-1, precision=None, chan_table=None,
                 chan_replay_period=0, csi_seed=0):
        L = lib()
        self.precision = precision or default_precision()
        if self.precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self._tx = _c(tx_pos, np.float64).reshape(-1, 3)
        self._fr = _c(carrier_freqs, np.float64)
        if self._tx.shape[0] != n_ant or self._fr.shape[0] != n_fft:
            raise ValueError("tx_pos must be [n_ant, 3] and carrier_freqs [n_fft]")
        self._tab = None
        if channel == "table":
            tab = np.asarray(chan_table, dtype=np.complex128)
            if tab.shape != (n_ant, n_fft):
                raise ValueError("chan_table must be the [n_ant, n_fft] channel matrix")
            self._tab = np.ascontiguousarray(tab).view(np.float64)
        cfg = MimoConfig(n_ant=n_ant, n_sub_carr=n_sub_carr, n_fft=n_fft, constel_size=constel_size, cp_len=cp_len,
                         channel_kind=CH_KINDS[channel], receiver_kind=RX_KINDS[receiver], device=device,
                         rx_loc_var=float(rx_loc_var), reroll_chan=int(bool(reroll)),
                         precision=PRECISIONS[self.precision],
                         tx_pos=_ptr(self._tx, ctypes.c_double), carrier_freqs=_ptr(self._fr, ctypes.c_double),
                         chan_table=_ptr(self._tab, ctypes.c_double) if self._tab is not None else None,
                         chan_replay_period=int(chan_replay_period), csi_seed=int(csi_seed))
        cfg.rx_pos[:] = [float(v) for v in rx_pos]
        h = L.mimo_engine_create(ctypes.byref(cfg))
        if not h:
            raise ValueError(L.mimo_last_error().decode())
        self._h, self._L = h, L   # the library this handle belongs to
        self.n_sub_carr, self.constel_size = n_sub_carr, constel_size
        self.n_fft = n_fft
        self.n_ant = n_ant

    @staticmethod
    def make_point(ibo_db, snr_db, avg_symbol_power, pa_kind, sat_pow=0.0, p_hardness=0.0, toi_coeff=0.0,
                   cnc_pa_kind=None, cnc_sat_pow=0.0, cnc_toi_coeff=0.0, cnc_alpha=1.0, csi_eps=None,
                   array_alpha=None):
        """A mimo_point from the per-point object state (Link.point_params() keys)."""
        return MimoPoint(ibo_db=float(ibo_db), snr_db=float(snr_db), avg_symbol_power=float(avg_symbol_power),
                         pa_kind=PA_KINDS[pa_kind], cnc_pa_kind=PA_KINDS[cnc_pa_kind or pa_kind],
                         sat_pow=float(sat_pow), p_hardness=float(p_hardness), toi_coeff=float(toi_coeff),
                         cnc_sat_pow=float(cnc_sat_pow), cnc_toi_coeff=float(cnc_toi_coeff),
                         cnc_alpha=float(cnc_alpha), csi_eps=-1.0 if csi_eps is None else float(csi_eps),
                         array_alpha=0.0 if array_alpha is None else float(array_alpha))

    def set_point(self, ibo_db, snr_db, avg_symbol_power, pa_kind, **kw):
        pt = self.make_point(ibo_db, snr_db, avg_symbol_power, pa_kind, **kw)
        _check(self._L.mimo_engine_set_point(self._h, ctypes.byref(pt)))
        self._point = pt  # the one-point measure() runs it

    def _points_call(self, name, points, seeds, first_trials, n_trials, iters, incl_clean, per_trial, rows=None,
                     tail=None):
        """Marshals a ``mimo_engine_*_points`` call and makes it (``name``: the C function).
        ``rows``: None for a plain run, else ``n_idx -> (shape of a point's row, the C arguments
        that stand ahead of the row pointers)``.  -> (err, bits, per-trial counts or None), for a
        row mode (err, bits, rows[P, *shape], per-trial counts, per-trial rows [sum n_trials, *shape]).
        ``tail``: ``(trials of the call, n_idx) -> the C arguments behind the row pointers``."""
        P = len(points)
        arr = (MimoPoint * max(1, P))()
        for i, pt in enumerate(points):
            arr[i] = pt if isinstance(pt, MimoPoint) else self.make_point(**pt)
        it = _c(sorted(set(int(i) for i in iters)), np.int32)
        n_idx = len(it) + (1 if incl_clean else 0)
        shape, lead = rows(n_idx) if rows else (None, ())
        sd = _c(np.asarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64).reshape(-1), np.uint64)
        ft = _c(np.asarray(first_trials, dtype=np.uint64).reshape(-1), np.uint64)
        nt = _c(np.asarray(n_trials, dtype=np.uint64).reshape(-1), np.uint64)
        if not (len(sd) == len(ft) == len(nt) == P):
            raise ValueError("points, seeds, first_trials and n_trials must have the same length")

        def out(shape, dtype, ctype, wanted=True):
            a = np.zeros(shape, dtype) if wanted else None
            return a, (_ptr(a, ctype) if wanted else None)

        err, p_err = out((P, n_idx), np.uint64, ctypes.c_uint64)
        bits, p_bits = out((P, n_idx), np.uint64, ctypes.c_uint64)
        pt, p_pt = out((int(nt.sum()), n_idx), np.uint32, ctypes.c_uint32, per_trial)
        args = [self._h, P, arr, _ptr(sd, ctypes.c_uint64), _ptr(ft, ctypes.c_uint64), _ptr(nt, ctypes.c_uint64),
                _ptr(it, ctypes.c_int32), len(it), int(bool(incl_clean)), p_err, p_bits, p_pt]
        if shape is None:
            _check(getattr(self._L, name)(*args))
            return err, bits, pt
        tot, p_tot = out((P,) + shape, np.float64, ctypes.c_double)
        pr, p_pr = out((int(nt.sum()),) + shape, np.float64, ctypes.c_double, per_trial)
        _check(getattr(self._L, name)(*args, *lead, p_tot, p_pr, *(tail(int(nt.sum()), n_idx) if tail else ())))
        return err, bits, tot, pt, pr

    def _one_point(self, point):
        """The point of a one-point row-mode call: ``point``, or the last set_point's."""
        if point is None:
            point = getattr(self, "_point", None)
            if point is None:
                raise EngineError("mimo_engine_set_point was not called")
        return point

    def run_points(self, points, seeds, first_trials, n_trials, iters, incl_clean=False, per_trial=False):
        """Many grid points in as few launches as possible (mimo_engine_run_points).
        points: list of dicts (make_point keywords) or MimoPoint.  -> (err[P, n_idx],
        bits[P, n_idx], per_trial[sum n_trials, n_idx] or None)."""
        return self._points_call("mimo_engine_run_points", points, seeds, first_trials, n_trials, iters, incl_clean,
                                 per_trial)

    def run(self, seed, first_trial, n_trials, iters, incl_clean=False, per_trial=False):
        """-> (err[n_idx], bits[n_idx], per_trial[n_trials, n_idx] or None)."""
        it = _c(sorted(set(int(i) for i in iters)), np.int32)
        n_idx = len(it) + (1 if incl_clean else 0)
        err = np.zeros(n_idx, np.uint64)
        bits = np.zeros(n_idx, np.uint64)
        pt = np.zeros((int(n_trials), n_idx), np.uint32) if per_trial else None
        _check(self._L.mimo_engine_run(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_trial), int(n_trials),
                                     _ptr(it, ctypes.c_int32), len(it), int(bool(incl_clean)),
                                     _ptr(err, ctypes.c_uint64), _ptr(bits, ctypes.c_uint64),
                                     _ptr(pt, ctypes.c_uint32) if pt is not None else None))
        return err, bits, pt

    def measure_points(self, points, seeds, first_trials, n_trials, iters, incl_clean=False, per_trial=False):
        """run_points in measure mode (mimo_engine_measure_points; float64 engines): the same
        trials and counts, and per point the row of signal / distortion power sums.
        -> (err[P, n_idx], bits[P, n_idx], meas[P, n_meas], per-trial counts [sum n_trials, n_idx]
        or None, per-trial rows [sum n_trials, n_meas] or None); SignalStats(meas[i], err[i], bits[i])."""
        return self._points_call("mimo_engine_measure_points", points, seeds, first_trials, n_trials, iters,
                                 incl_clean, per_trial, lambda n_idx: ((MEAS_FIXED + n_idx,), ()))

    def measure(self, seed, first_trial, n_trials, iters, incl_clean=False, per_trial=False, point=None):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], meas[n_meas], per-trial counts or None, per-trial rows or None)."""
        err, bits, meas, pt, pm = self.measure_points([self._one_point(point)], [seed], [first_trial], [n_trials],
                                                      iters, incl_clean, per_trial)
        return err[0], bits[0], meas[0], pt, pm

    def spectrum_points(self, points, seeds, first_trials, n_trials, iters, incl_clean=False, per_trial=False):
        """run_points in spectrum mode (mimo_engine_spectrum_points; float64 engines): the same
        trials and counts, and per point the row of the array's radiated PSD per FFT bin, Ex and C.
        -> (err[P, n_idx], bits[P, n_idx], spec[P, n_spec], per-trial counts [sum n_trials, n_idx]
        or None, per-trial rows [sum n_trials, n_spec] or None); SpectrumStats(spec[i], n_sub_carr)."""
        return self._points_call("mimo_engine_spectrum_points", points, seeds, first_trials, n_trials, iters,
                                 incl_clean, per_trial, lambda n_idx: ((self.n_fft + SPEC_FIXED,), ()))

    def spectrum(self, seed, first_trial, n_trials, iters, incl_clean=False, per_trial=False, point=None):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], spec[n_spec], per-trial counts or None, per-trial rows or None)."""
        err, bits, spec, pt, ps = self.spectrum_points([self._one_point(point)], [seed], [first_trial], [n_trials],
                                                       iters, incl_clean, per_trial)
        return err[0], bits[0], spec[0], pt, ps

    def beam_points(self, points, seeds, first_trials, n_trials, iters, probes, incl_clean=False, per_trial=False):
        """run_points in beam mode (mimo_engine_beam_points; float64 engines): the same trials and
        counts, and per point and probe position (``probes``: [n_probes, 3] in metres, the same for
        every point) the row ``[Py_in, Py_oob, Px, Re C, Im C]``.
        -> (err[P, n_idx], bits[P, n_idx], beam[P, n_probes, 5], per-trial counts [sum n_trials, n_idx]
        or None, per-trial rows [sum n_trials, n_probes, 5] or None); BeamStats(beam[i])."""
        def rows(n_idx):
            pr = _c(probes, np.float64)
            if pr.ndim != 2 or pr.shape[1] != 3:
                raise ValueError("probes must be [n_probes, 3]")
            return (pr.shape[0], BEAM_FIXED), (_ptr(pr, ctypes.c_double), pr.shape[0])

        return self._points_call("mimo_engine_beam_points", points, seeds, first_trials, n_trials, iters, incl_clean,
                                 per_trial, rows)

    def beam(self, seed, first_trial, n_trials, iters, probes, incl_clean=False, per_trial=False, point=None):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], beam[n_probes, 5], per-trial counts or None, per-trial rows or None)."""
        err, bits, beam, pt, pb = self.beam_points([self._one_point(point)], [seed], [first_trial], [n_trials], iters,
                                                   probes, incl_clean, per_trial)
        return err[0], bits[0], beam[0], pt, pb

    def envelope_points(self, points, seeds, first_trials, n_trials, iters, ref_pow, incl_clean=False,
                        per_trial=False):
        """run_points in envelope mode (mimo_engine_envelope_points; float64 engines): the same trials
        and counts, and per point the row of the two instantaneous-power histograms (PA input and
        output, bins relative to ``ref_pow``), Pin, Pout and C.
        -> (err[P, n_idx], bits[P, n_idx], env[P, 260], per-trial counts [sum n_trials, n_idx] or None,
        per-trial rows [sum n_trials, 260] or None); EnvelopeStats(env[i], n_ant, n_fft, n_trials[i], ref_pow)."""
        return self._points_call("mimo_engine_envelope_points", points, seeds, first_trials, n_trials, iters,
                                 incl_clean, per_trial, lambda n_idx: ((ENV_WIDTH,), (ctypes.c_double(float(ref_pow)),)))

    def envelope(self, seed, first_trial, n_trials, iters, ref_pow, incl_clean=False, per_trial=False, point=None):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], env[260], per-trial counts or None, per-trial rows or None)."""
        err, bits, env, pt, pe = self.envelope_points([self._one_point(point)], [seed], [first_trial], [n_trials],
                                                      iters, ref_pow, incl_clean, per_trial)
        return err[0], bits[0], env[0], pt, pe

    def soft_points(self, points, seeds, first_trials, n_trials, iters, rho_max, incl_clean=False, per_trial=False):
        """run_points in soft mode (mimo_engine_soft_points; float64 engines): the same trials and
        counts, and per point and counter index the histogram of the bit reliabilities over 256 bins
        of width ``rho_max / 128``.
        -> (err[P, n_idx], bits[P, n_idx], soft[P, n_idx, 256], per-trial counts [sum n_trials, n_idx] or
        None, per-trial rows [sum n_trials, n_idx, 256] or None);
        SoftStats(soft[i], rho_max, constel_size, n_trials[i])."""
        return self._points_call("mimo_engine_soft_points", points, seeds, first_trials, n_trials, iters, incl_clean,
                                 per_trial, lambda n_idx: ((n_idx, SOFT_BINS), (ctypes.c_double(float(rho_max)),)))

    def soft(self, seed, first_trial, n_trials, iters, rho_max, incl_clean=False, per_trial=False, point=None):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], soft[n_idx, 256], per-trial counts or None, per-trial rows or None)."""
        err, bits, soft, pt, ps = self.soft_points([self._one_point(point)], [seed], [first_trial], [n_trials],
                                                   iters, rho_max, incl_clean, per_trial)
        return err[0], bits[0], soft[0], pt, ps

    def coded_codewords(self, code):
        """n_cw: codewords per trial and counter index (mimo_coded_codewords)."""
        return coded_codewords(self.n_sub_carr, self.constel_size, code)

    def coded_points(self, points, seeds, first_trials, n_trials, iters, code, rho_max, incl_clean=False,
                     per_trial=False, chan=False):
        """run_points in coded mode (mimo_engine_coded_points; float64 engines): the same trials and
        counts, and per point and counter index the four error counts of the LDPC-coded link
        (``code``: an ``LdpcCode``; channel values quantised over ``+-rho_max``).
        -> (err[P, n_idx], bits[P, n_idx], coded[P, n_idx, 4], per-trial counts [sum n_trials, n_idx] or
        None, per-trial rows [sum n_trials, n_idx, 4] or None), with ``chan=True`` also the channel
        values [sum n_trials, n_idx, S log2 M] int8;
        CodedStats(coded[i], n_trials[i] * coded_codewords(code), code.n_bits)."""
        sb = self.n_sub_carr * int(round(np.log2(self.constel_size)))
        got = []

        def tail(n, n_idx):
            got.append(np.zeros((n, n_idx, sb), np.int8) if chan else None)
            return (_ptr(got[0], ctypes.c_int8) if chan else None,)

        out = self._points_call("mimo_engine_coded_points", points, seeds, first_trials, n_trials, iters, incl_clean,
                                per_trial, lambda n_idx: ((n_idx, CODED_FIXED), (ctypes.byref(code),
                                                                                 ctypes.c_double(float(rho_max)))),
                                tail)
        return out + (got[0],) if chan else out

    def coded(self, seed, first_trial, n_trials, iters, code, rho_max, incl_clean=False, per_trial=False, point=None,
              chan=False):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], coded[n_idx, 4], per-trial counts or None, per-trial rows or None
        [, channel values])."""
        out = self.coded_points([self._one_point(point)], [seed], [first_trial], [n_trials], iters, code, rho_max,
                                incl_clean, per_trial, chan)
        return (out[0][0], out[1][0], out[2][0]) + tuple(out[3:])

    def turbo_points(self, points, seeds, first_trials, n_trials, iters, code, rho_max, n_passes, incl_clean=False,
                     per_trial=False, chan=False, z=False):
        """run_points in turbo mode (mimo_engine_turbo_points; float64 CNC engines): the same trials and
        counts, and per point and pass of the decoder-aided CNC receiver the four error counts of the
        LDPC-coded link (``code``: an ``LdpcCode``; channel values quantised over ``+-rho_max``).
        -> (err[P, n_idx], bits[P, n_idx], turbo[P, n_passes, 4], per-trial counts [sum n_trials, n_idx] or
        None, per-trial rows [sum n_trials, n_passes, 4] or None), with ``chan=True`` also the channel
        values [sum n_trials, n_passes, S log2 M] int8 and with ``z=True`` the received vectors
        [sum n_trials, S] complex128;
        TurboStats(turbo[i], n_trials[i] * coded_codewords(code), code.n_bits)."""
        sb = self.n_sub_carr * int(round(np.log2(self.constel_size)))
        n_passes = int(n_passes)
        # (a number out of range is the library's to refuse: the arrays then hold one pass at least, so
        # that the refusal names n_passes and no empty array's pointer)
        shape_p = max(1, min(n_passes, TURBO_MAX_PASSES))
        got = []

        def tail(n, n_idx):
            got.append(np.zeros((n, shape_p, sb), np.int8) if chan else None)
            got.append(np.zeros((n, self.n_sub_carr), np.complex128) if z else None)
            return (_ptr(got[0], ctypes.c_int8) if chan else None,
                    _ptr(got[1].view(np.float64), ctypes.c_double) if z else None)

        out = self._points_call("mimo_engine_turbo_points", points, seeds, first_trials, n_trials, iters, incl_clean,
                                per_trial, lambda n_idx: ((shape_p, CODED_FIXED),
                                                          (ctypes.byref(code) if code is not None else None,
                                                           ctypes.c_double(float(rho_max)), ctypes.c_int32(n_passes))),
                                tail)
        return out + ((got[0],) if chan else ()) + ((got[1],) if z else ())

    def turbo(self, seed, first_trial, n_trials, iters, code, rho_max, n_passes, incl_clean=False, per_trial=False,
              point=None, chan=False, z=False):
        """One point (the last set_point's, or ``point``: make_point keywords / MimoPoint).
        -> (err[n_idx], bits[n_idx], turbo[n_passes, 4], per-trial counts or None, per-trial rows or None
        [, channel values][, received vectors])."""
        out = self.turbo_points([self._one_point(point)], [seed], [first_trial], [n_trials], iters, code, rho_max,
                                n_passes, incl_clean, per_trial, chan, z)
        return (out[0][0], out[1][0], out[2][0]) + tuple(out[3:])

    def cnc_step(self, z, labels, point=None):
        """The turbo mode's step kernel on caller-given vectors (mimo_engine_cnc_step): ``z`` [n, S]
        complex and the decided ``labels`` [n, S] in [0, M) -> ``v = z - dist`` [n, S] complex128, dist the
        clipping distortion the receiver's PA model (the point's ``cnc_*`` fields) gives the decided
        symbols.  ``point``: make_point keywords / MimoPoint, or the last set_point's."""
        pt = self._one_point(point)
        pt = pt if isinstance(pt, MimoPoint) else self.make_point(**pt)
        zz = np.ascontiguousarray(np.asarray(z, np.complex128).reshape(-1, self.n_sub_carr))
        lab = _c(np.asarray(labels).reshape(-1, self.n_sub_carr), np.int32)
        if lab.shape != zz.shape:
            raise ValueError("z and labels must both be [n, n_sub_carr]")
        out = np.zeros(zz.shape, np.complex128)
        _check(self._L.mimo_engine_cnc_step(self._h, ctypes.byref(pt), _ptr(zz.view(np.float64), ctypes.c_double),
                                            _ptr(lab, ctypes.c_int32), zz.shape[0],
                                            _ptr(out.view(np.float64), ctypes.c_double)))
        return out

    @property
    def chan_kernel_ms(self):
        """Device time of the TDL generator kernels of the last call [ms] (0 unless channel="tdl")."""
        return self._L.mimo_engine_last_chan_ms(self._h)

    def set_channel_bank(self, tables):
        """A channel bank for a ``channel="table"`` engine (mimo_engine_set_channel_bank): ``tables``
        [n_bank, n_ant, n_fft] complex, and from then on trial i of every run uses table
        ``i % n_bank``.  ``None`` or an empty bank: back to the create-time table.  Copied; uploaded
        at the next run."""
        if tables is None:
            tab = np.zeros((0, self.n_ant, self.n_fft), np.complex128)
        else:
            tab = np.asarray(tables, dtype=np.complex128)
        if tab.ndim != 3 or tab.shape[1:] != (self.n_ant, self.n_fft):
            raise ValueError("tables must be [n_bank, n_ant, n_fft] channel matrices")
        iq = np.ascontiguousarray(tab).view(np.float64)
        _check(self._L.mimo_engine_set_channel_bank(self._h, tab.shape[0], _ptr(iq, ctypes.c_double) if tab.size else None))

    def set_tdl(self, delays, powers, ant_amp=None):
        """The power-delay profile of a ``channel="tdl"`` engine (mimo_engine_set_tdl): whole-sample
        ``delays``, linear ``powers`` and, optionally, an amplitude per antenna.  Copied."""
        if ant_amp is not None and np.size(ant_amp) != self.n_ant:
            raise ValueError("ant_amp must hold n_ant amplitudes")
        prof = TdlProfile(delays, powers, ant_amp)
        _check(self._L.mimo_engine_set_tdl(self._h, ctypes.byref(prof)))

    def set_rays(self, delays, ray_tap, ray_amp, steer, ray_kind=None):
        """The ray-cluster profile of a ``channel="tdl"`` engine (mimo_engine_set_rays): tap
        ``delays``, the tap and amplitude of every ray, ``steer`` [n_ant, R] complex and, optionally,
        the rays' kinds (0 diffuse, 1 specular).  Copied; it replaces a ``set_tdl`` profile and the
        other way round."""
        prof = RayProfile(delays, ray_tap, ray_amp, steer, ray_kind)
        if prof.n_ant != self.n_ant:
            raise ValueError("steer must be [n_ant, n_rays]")
        _check(self._L.mimo_engine_set_rays(self._h, ctypes.byref(prof)))

    @property
    def decode_kernel_ms(self):
        """Device time of the decoder kernels of the last coded call, or of the whole pass loop (step
        kernels and decoders) of the last turbo call (0 after any other call)."""
        return self._L.mimo_engine_last_decode_ms(self._h)

    @property
    def kernel_ms(self):
        return self._L.mimo_engine_last_kernel_ms(self._h)

    @property
    def beam_kernel_ms(self):
        """Device time of the beamforming kernels of the last beam call."""
        return self._L.mimo_engine_last_beam_ms(self._h)

    def describe(self):
        return self._L.mimo_engine_describe(self._h).decode()

    def close(self):
        if getattr(self, "_h", None):
            self._L.mimo_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ fine-seam helpers
def qam_map(constel_size, labels):
    lab = _c(labels, np.int32).reshape(-1)
    out = np.empty(lab.size, np.complex128)
    _check(lib().mimo_qam_map(int(constel_size), _ptr(lab, ctypes.c_int32), lab.size,
                              _ptr(out.view(np.float64), ctypes.c_double)))
    return out


def qam_slice(constel_size, symbols):
    z = as_iq(np.asarray(symbols).reshape(-1))
    out = np.empty(z.size // 2, np.int32)
    _check(lib().mimo_qam_slice(int(constel_size), _ptr(z, ctypes.c_double), out.size, _ptr(out, ctypes.c_int32)))
    return out.astype(np.int64)


def qam_llr(constel_size, symbols, noise_var):
    z = as_iq(np.asarray(symbols).reshape(-1))
    n = z.size // 2
    nv = _c(np.broadcast_to(np.asarray(noise_var, np.float64), (n,)), np.float64)
    nb = int(np.log2(constel_size))
    out = np.empty(n * nb, np.float64)
    _check(lib().mimo_qam_llr(int(constel_size), _ptr(z, ctypes.c_double), n, _ptr(nv, ctypes.c_double),
                              _ptr(out, ctypes.c_double)))
    return out


def qam_softbits(constel_size, symbols):
    """The soft mode's max-log soft bits ``lambda`` (mimo_qam_softbits): [n][log2 M], the I-axis bits
    MSB first and then the Q-axis bits (``qam_llr``'s layout); ``4 lambda / noise_var`` approximates it."""
    z = as_iq(np.asarray(symbols).reshape(-1))
    n = z.size // 2
    nb = int(np.log2(constel_size))
    out = np.empty(n * nb, np.float64)
    _check(lib().mimo_qam_softbits(int(constel_size), _ptr(z, ctypes.c_double), n, _ptr(out, ctypes.c_double)))
    return out.reshape(n, nb)


def coded_width(n_iters, incl_clean=False):
    """Doubles of a coded row (mimo_coded_width): 4 per counter index."""
    n = lib().mimo_coded_width(int(n_iters), int(bool(incl_clean)))
    if n < 0:
        _check(n)
    return n


def turbo_width(n_passes):
    """Doubles of a turbo row (mimo_turbo_width): 4 per pass, ``n_passes`` in [1, 16]."""
    n = lib().mimo_turbo_width(int(n_passes))
    if n < 0:
        _check(n)
    return n


def coded_codewords(n_sub_carr, constel_size, code):
    """n_cw = floor(n_sub_carr log2(constel_size) / N): the codewords of one trial and counter index
    (mimo_coded_codewords; raises for a code that breaks its rules or is longer than a trial)."""
    n = lib().mimo_coded_codewords(int(n_sub_carr), int(constel_size), ctypes.byref(code) if code is not None else None)
    if n < 0:
        _check(n)
    return n


def ldpc_decode(code, chan):
    """The coded mode's decoder (mimo_ldpc_decode) on channel values ``chan`` [n_cw, N] (integers with
    ``|c| <= 63``) -> the final L of every bit, [n_cw, N] int16; a bit is decided 1 where L < 0."""
    c = np.asarray(chan)
    if c.size and np.abs(c).max() > 127:
        raise EngineError("chan must be in [-63, 63]")
    c = _c(c, np.int8).reshape(-1)
    n = code.n_bits
    if n > 0 and c.size % n:
        raise ValueError("chan must hold whole codewords of n_cols z values")
    n_cw = c.size // n if n > 0 else 0   # (a code without bits is the library's to refuse)
    out = np.zeros(c.size, np.int16)
    _check(lib().mimo_ldpc_decode(ctypes.byref(code), _ptr(c, ctypes.c_int8), n_cw, _ptr(out, ctypes.c_int16)))
    return out.reshape(n_cw, n) if n > 0 else out


def bank_capacity(n_ant, n_sub_carr, precision="f64"):
    """Entries a channel bank holds (mimo_bank_capacity): what fits MIMO_BANK_BUFFER_BYTES; also
    the trials of one launch of a ``channel="tdl"`` engine.  Host only."""
    n = lib().mimo_bank_capacity(int(n_ant), int(n_sub_carr), PRECISIONS[precision])
    if n < 0:
        raise ValueError(lib().mimo_last_error().decode())
    return int(n)


def tdl_channels(delays, powers, n_ant, n_fft, seed, first_trial, n, ant_amp=None, taps=False):
    """The TDL engine's channel realisations on host arrays (mimo_tdl_channels): trials
    ``first_trial ... first_trial + n - 1`` under the key ``seed``, by the engine's own generator.
    -> H [n, n_ant, n_fft] complex (numpy.fft bin order), with ``taps=True`` (H, taps [n, n_ant, L])."""
    if ant_amp is not None and np.size(ant_amp) != n_ant:
        raise ValueError("ant_amp must hold n_ant amplitudes")
    prof = TdlProfile(delays, powers, ant_amp)
    n = int(n)
    h = np.zeros((max(n, 0), n_ant, n_fft), np.complex128)
    g = np.zeros((max(n, 0), n_ant, prof.n_taps), np.complex128) if taps else None
    _check(lib().mimo_tdl_channels(ctypes.byref(prof), int(n_ant), int(n_fft), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   int(first_trial) & 0xFFFFFFFFFFFFFFFF, n, _ptr(h.view(np.float64), ctypes.c_double),
                                   _ptr(g.view(np.float64), ctypes.c_double) if taps else None))
    return (h, g) if taps else h


def rays_channels(delays, ray_tap, ray_amp, steer, n_fft, seed, first_trial, n, ray_kind=None, taps=False, gains=False):
    """The realisations of a ray-cluster profile on host arrays (mimo_rays_channels), by the engine's
    own generator: trials ``first_trial ... first_trial + n - 1`` under the key ``seed``; ``n_ant`` is
    ``steer``'s first dimension.  -> H [n, n_ant, n_fft] complex (numpy.fft bin order); with
    ``taps=True`` and / or ``gains=True`` a tuple (H[, taps [n, n_ant, L]][, gains [n, R]])."""
    prof = RayProfile(delays, ray_tap, ray_amp, steer, ray_kind)
    n, n_ant = int(n), prof.n_ant
    h = np.zeros((max(n, 0), n_ant, n_fft), np.complex128)
    g = np.zeros((max(n, 0), n_ant, prof.n_taps), np.complex128) if taps else None
    c = np.zeros((max(n, 0), prof.n_rays), np.complex128) if gains else None
    _check(lib().mimo_rays_channels(ctypes.byref(prof), n_ant, int(n_fft), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                    int(first_trial) & 0xFFFFFFFFFFFFFFFF, n, _ptr(h.view(np.float64), ctypes.c_double),
                                    _ptr(g.view(np.float64), ctypes.c_double) if taps else None,
                                    _ptr(c.view(np.float64), ctypes.c_double) if gains else None))
    out = (h,) + ((g,) if taps else ()) + ((c,) if gains else ())
    return out if len(out) > 1 else h


def fft(x, inverse=False):
    x = np.asarray(x, np.complex128)
    shape = x.shape
    xi = as_iq(x.reshape(-1, shape[-1]))
    out = np.empty(x.size, np.complex128)
    _check(lib().mimo_fft(shape[-1], x.size // shape[-1], int(inverse), _ptr(xi, ctypes.c_double),
                          _ptr(out.view(np.float64), ctypes.c_double)))
    return out.reshape(shape)


def ofdm_tx(symbols, n_fft, n_sub_carr, cp_len):
    s = np.asarray(symbols, np.complex128)
    if s.shape[-1] != n_sub_carr:
        raise ValueError("mod_symbols length must match n_sub_carr value")
    batch = s.size // n_sub_carr
    out = np.empty(batch * (n_fft + cp_len), np.complex128)
    _check(lib().mimo_ofdm_tx(n_fft, n_sub_carr, cp_len, batch, _ptr(as_iq(s), ctypes.c_double),
                              _ptr(out.view(np.float64), ctypes.c_double)))
    return out.reshape(s.shape[:-1] + (n_fft + cp_len,))


def ofdm_rx(td, n_fft, n_sub_carr, cp_len):
    t = np.asarray(td, np.complex128)
    if t.ndim < 1 or t.shape[-1] != n_fft + cp_len:
        raise ValueError("the last axis of td must have n_fft + cp_len samples")
    batch = t.size // (n_fft + cp_len)
    out = np.empty(batch * n_sub_carr, np.complex128)
    _check(lib().mimo_ofdm_rx(n_fft, n_sub_carr, cp_len, batch, _ptr(as_iq(t), ctypes.c_double),
                              _ptr(out.view(np.float64), ctypes.c_double)))
    return out.reshape(t.shape[:-1] + (n_sub_carr,))


def pa(kind, x, sat_pow=0.0, p_hardness=0.0, toi_coeff=0.0):
    xa = np.asarray(x)
    is_real = not np.iscomplexobj(xa)
    x2 = np.asarray(xa, np.complex128)
    out = np.empty(x2.size, np.complex128)
    _check(lib().mimo_pa(PA_KINDS[kind], float(sat_pow), float(p_hardness), float(toi_coeff),
                         _ptr(as_iq(x2.reshape(-1)), ctypes.c_double), x2.size,
                         _ptr(out.view(np.float64), ctypes.c_double)))
    out = out.reshape(x2.shape)
    return out.real.copy() if is_real else out


def calc_alpha(ibo_db):
    """Bussgang gain per IBO [dB] by the float64 kernels' segment table (alpha_fit.h)."""
    ibo = np.ascontiguousarray(np.atleast_1d(np.asarray(ibo_db, np.float64)))
    out = np.empty(ibo.size, np.float64)
    _check(lib().mimo_calc_alpha(_ptr(ibo, ctypes.c_double), ibo.size, _ptr(out, ctypes.c_double)))
    return out.reshape(np.shape(ibo_db))


def mrt_precode(h_sc):
    h = np.asarray(h_sc, np.complex128)
    if h.ndim != 2:
        raise ValueError("h_sc must be a 2-D [n_ant, n_cols] matrix")
    A, K = h.shape
    out = np.empty(A * K, np.complex128)
    _check(lib().mimo_mrt_precode(A, K, _ptr(as_iq(h), ctypes.c_double), _ptr(out.view(np.float64), ctypes.c_double)))
    return out.reshape(A, K)


def combine(h, y):
    h = np.asarray(h, np.complex128)
    y = np.asarray(y, np.complex128)
    if h.ndim != 2 or h.shape != y.shape:
        raise ValueError("h and y must be 2-D [n_ant, n] matrices of the same shape")
    A, K = h.shape
    out = np.empty(K, np.complex128)
    _check(lib().mimo_combine(A, K, _ptr(as_iq(h), ctypes.c_double), _ptr(as_iq(y), ctypes.c_double),
                              _ptr(out.view(np.float64), ctypes.c_double)))
    return out


def awgn(x, noise_std, seed, counter):
    xa = np.asarray(x, np.complex128)
    out = np.empty(xa.size, np.complex128)
    _check(lib().mimo_awgn(int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter), xa.size, float(noise_std),
                           _ptr(as_iq(xa.reshape(-1)), ctypes.c_double), _ptr(out.view(np.float64), ctypes.c_double)))
    return out.reshape(xa.shape)


def count_bit_errors(a, b):
    a = _c(a, np.int64).reshape(-1)
    b = _c(b, np.int64).reshape(-1)
    if a.size != b.size:
        raise ValueError("a and b must have the same number of elements")
    out = np.zeros(1, np.int64)
    _check(lib().mimo_count_bit_errors(_ptr(a, ctypes.c_int64), _ptr(b, ctypes.c_int64), a.size,
                                       _ptr(out, ctypes.c_int64)))
    return int(out[0])


def cnc_receive(constel_size, n_fft, pa_kind, sat_pow, p_hardness, toi_coeff, alpha, iters, rx_sc, return_bits=True):
    """{iteration: detected labels}, or with ``return_bits=False`` {iteration: the corrected
    slicer input rx - d} (mimo_cnc_receive_ex)."""
    z = as_iq(np.asarray(rx_sc).reshape(-1))
    S = z.size // 2
    it = _c(sorted(set(int(i) for i in iters)), np.int32)
    lab = np.empty((len(it), S), np.int32) if return_bits else None
    cor = None if return_bits else np.empty((len(it), S), np.complex128)
    _check(lib().mimo_cnc_receive_ex(int(constel_size), int(n_fft), S, PA_KINDS[pa_kind], float(sat_pow),
                                     float(p_hardness), float(toi_coeff), float(alpha), _ptr(it, ctypes.c_int32),
                                     len(it), _ptr(z, ctypes.c_double),
                                     _ptr(lab, ctypes.c_int32) if lab is not None else None,
                                     _ptr(cor.view(np.float64), ctypes.c_double) if cor is not None else None))
    if return_bits:
        return {int(i): lab[j].astype(np.int64) for j, i in enumerate(it)}
    return {int(i): cor[j] for j, i in enumerate(it)}
