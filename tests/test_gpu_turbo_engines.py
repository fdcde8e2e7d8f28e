"""The turbo mode on the other engines and next to the other modes: a ``channel="tdl"`` engine gives
the rows of a bank engine that holds the generator seam's matrices, a turbo call before and after
calls of other modes on one engine returns a fresh engine's bits (the property of
tests/test_gpu_mode_sequence.py for the eighth mode), and ``Link.turbo`` equals the engine call.
"""
import numpy as np
import pytest

from gpu_util import engine_for
from test_gpu_mode_sequence import CFG, CODE, ITERS, OTHER_CODE, RHO_MAX, SEED
from test_gpu_mode_sequence import call as other_call
from test_gpu_mode_sequence import new_fresh as other_fresh
from test_gpu_tdl import bank_of_seam, tdl_cfg, tdl_engine

pytestmark = pytest.mark.gpu

N_PASSES = 3


def turbo_call(eng, first, n, code=CODE, chan=True):
    return eng.turbo(SEED, first, n, ITERS, code, RHO_MAX, N_PASSES, incl_clean=True, per_trial=True, chan=chan, z=chan)


def turbo_fresh(first, n, code=CODE, chan=True):
    eng = engine_for(CFG, precision="f64")
    out = turbo_call(eng, first, n, code, chan)
    eng.close()
    return out


def assert_same(got, want, label):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g is not None and g.shape[0] > 0
        np.testing.assert_array_equal(g, w, err_msg=f"{label} output {k}")


def test_tdl_engine_gives_the_rows_of_a_bank_engine_on_the_seams_matrices():
    cfg = tdl_cfg(4, 100, 256, M=64)
    eng, ref = tdl_engine(cfg, "f64"), bank_of_seam(cfg, "f64", 31, 7, 5)
    got = eng.turbo(31, 7, 5, ITERS, CODE, 8.0, N_PASSES, incl_clean=True, per_trial=True, chan=True, z=True)
    assert eng.chan_kernel_ms > 0 and eng.decode_kernel_ms > 0
    want = ref.turbo(31, 7, 5, ITERS, CODE, 8.0, N_PASSES, incl_clean=True, per_trial=True, chan=True, z=True)
    eng.close()
    ref.close()
    assert_same(got, want, "tdl vs bank")
    assert got[2][:, 0].sum() > 0  # there are channel errors to feed back


@pytest.mark.parametrize("other", ["plain", "soft", "coded", "beam"])
def test_turbo_between_the_other_modes_equals_fresh_engines(other, monkeypatch):
    want = {(0, 11): turbo_fresh(0, 11), (16, 5): turbo_fresh(16, 5)}
    want_other = other_fresh(other, 16, 7)
    eng = engine_for(CFG, precision="f64")
    assert_same(turbo_call(eng, 0, 11), want[(0, 11)], f"turbo before {other}")
    assert eng.decode_kernel_ms > 0 and eng.beam_kernel_ms == 0
    assert_same(other_call(eng, other, 16, 7), want_other, f"{other} after turbo")
    assert (eng.decode_kernel_ms > 0) == (other == "coded")
    assert_same(turbo_call(eng, 16, 5), want[(16, 5)], f"turbo after {other}")
    if other == "coded":
        # another code, and a call without the optional outputs (one stream buffer), then the first again
        assert_same(turbo_call(eng, 0, 11, OTHER_CODE), turbo_fresh(0, 11, OTHER_CODE), "turbo with another code")
        assert_same(turbo_call(eng, 0, 11, chan=False), want[(0, 11)][:5], "turbo without the optional outputs")
        assert_same(turbo_call(eng, 0, 11), want[(0, 11)], "turbo after another code")
    monkeypatch.setenv("MIMO_MAX_LAUNCH_TRIALS", "3")  # four launches a call, in buffers that were larger
    assert_same(turbo_call(eng, 0, 11), want[(0, 11)], "turbo in four launches")
    eng.close()


def test_link_turbo_equals_engine_call():
    from link_util import build_link
    from mp_model import _seed64
    link, _ = build_link()  # A 8, S 64, F 128, 16-QAM, soft limiter at IBO 1: 256 bits a trial
    link.set_snr(14.0)
    nominal = link.nominal_llr_scale()
    st = link.turbo(True, [11, 22, 33], 8, CODE, N_PASSES)
    assert (st.n_passes, st.n_frames, st.n_code_bits, st.n_bits) == (N_PASSES, 2 * 8, 96, 192 * 8)
    eng = link.engine()
    _, _, turbo, _, _ = eng.turbo(_seed64([11, 22, 33]), 0, 8, [0], CODE, 32.0 / nominal, N_PASSES,
                                  point=link.point_params())
    np.testing.assert_array_equal(st.cells, turbo)
    # pass 0 is the coded call's iteration 0
    np.testing.assert_array_equal(link.coded(False, True, [0], [11, 22, 33], 8, CODE).cells[0], st.cells[0])
    # turbo_points at two IBOs: point 0 is the call above
    p0 = dict(link.point_params())
    link.update_distortion(4.0)
    p1 = dict(link.point_params())
    both = link.turbo_points(True, [[11, 22, 33], [5]], [p0, p1], 8, CODE, N_PASSES)
    np.testing.assert_array_equal(both[0].cells, st.cells)
    assert both[1].n_frames == st.n_frames
