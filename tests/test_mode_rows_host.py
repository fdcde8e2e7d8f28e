"""A run mode's rows, described once, on a machine without a GPU: every ``mimo_*_width`` function
agrees with the trailing dimensions the Python binding allocates for that mode, and an iteration
list that a plain run refuses is refused with the same words by every row mode, before its width or
the size of a launch is formed.  A call of no points validates and allocates, and makes no HIP call.
"""
import ctypes

import numpy as np
import pytest

import _engine
from utilities import qc_ldpc_code

MODES = ("measure", "spectrum", "beam", "envelope", "soft", "coded")
RHO_MAX = 16.0
CODE = qc_ldpc_code(16, 3, 6)  # 96 code bits: they fit the 128 bits of the smallest band below


def engine(n_fft):
    return _engine.Engine(n_ant=4, n_sub_carr=n_fft // 4, n_fft=n_fft, constel_size=16, cp_len=16, channel="rayleigh",
                          receiver="cnc", tx_pos=np.zeros((4, 3)), rx_pos=(0.0, 0.0, 0.0), rx_loc_var=10.0,
                          carrier_freqs=np.full(n_fft, 3.5e9), precision="f64")


def allocated(eng, mode, iters, incl_clean, probes):
    """The trailing dimensions of the rows the binding allocates for a call of no points."""
    none = ([], [], [], [])
    extra = {"beam": (probes,), "envelope": (1.0,), "soft": (RHO_MAX,), "coded": (CODE, RHO_MAX)}.get(mode, ())
    out = getattr(eng, mode + "_points")(*none, iters, *extra, incl_clean=incl_clean, per_trial=True)
    assert out[2].shape[0] == out[4].shape[0] == 0 and out[2].shape[1:] == out[4].shape[1:]
    return out[2].shape[1:]


@pytest.mark.parametrize("n_fft", [128, 8192])
@pytest.mark.parametrize("n_probes", [1, 4096])
@pytest.mark.parametrize("incl_clean", [False, True])
@pytest.mark.parametrize("n_iters", [1, 32])
def test_width_functions_agree_with_the_rows_the_binding_allocates(n_iters, incl_clean, n_probes, n_fft):
    lib = _engine.lib()
    assert lib.mimo_beam_width(4097) == -1  # 4096 is the most
    width = {"measure": lib.mimo_measure_width(n_iters, int(incl_clean)),
             "spectrum": lib.mimo_spectrum_width(n_fft),
             "beam": lib.mimo_beam_width(n_probes),
             "envelope": lib.mimo_envelope_width(),
             "soft": lib.mimo_soft_width(n_iters, int(incl_clean)),
             "coded": lib.mimo_coded_width(n_iters, int(incl_clean))}
    eng = engine(n_fft)
    for mode in MODES:
        shape = allocated(eng, mode, range(n_iters), incl_clean, np.ones((n_probes, 3)))
        assert width[mode] == int(np.prod(shape)) > 0, (mode, width[mode], shape)
    eng.close()


def points_call(lib, h, mode, iters):
    """The mode's ``mimo_engine_*_points`` call of no points with the iteration list as it stands
    (the binding would sort it) -> (return code, message)."""
    it = np.asarray(iters, np.int32)
    n_idx = max(1, len(iters)) + 1
    err, bits = np.zeros(n_idx, np.uint64), np.zeros(n_idx, np.uint64)
    rows = np.zeros(n_idx * 8192, np.float64)
    u64, dbl = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    args = [h, 0, None, None, None, None, it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(it), 1,
            err.ctypes.data_as(u64), bits.ctypes.data_as(u64), None]
    probes = np.ones((3, 3))
    lead = {"beam": (probes.ctypes.data_as(dbl), 3), "envelope": (ctypes.c_double(1.0),),
            "soft": (ctypes.c_double(RHO_MAX),), "coded": (ctypes.byref(CODE), ctypes.c_double(RHO_MAX))}.get(mode, ())
    if mode != "run":
        args += [*lead, rows.ctypes.data_as(dbl), None] + ([None] if mode == "coded" else [])
    rc = getattr(lib, "mimo_engine_%s_points" % mode)(*args)
    assert not err.any() and not bits.any() and not rows.any()
    return rc, lib.mimo_last_error().decode()


@pytest.mark.parametrize("iters,msg", [
    ([2, 1], "sorted and unique"),
    ([1, 1], "sorted and unique"),
    ([32], "[0, 31]"),
    ([-1], "[0, 31]"),
    ([], "at least one iteration"),
    (list(range(33)), "[0, 31]"),   # more indices than a row has columns for
    (list(range(32)) + [31], "sorted and unique"),
])
def test_a_refused_iteration_list_is_refused_alike_in_every_mode(iters, msg):
    lib = _engine.lib()
    eng = engine(256)
    rc, plain = points_call(lib, eng._h, "run", iters)
    assert rc == -1 and msg in plain
    for mode in MODES:
        assert points_call(lib, eng._h, mode, iters) == (-1, plain), mode
    assert points_call(lib, eng._h, "run", [0, 31])[0] == 0
    for mode in MODES:
        assert points_call(lib, eng._h, mode, [0, 31])[0] == 0, mode
    eng.close()
