"""The soft-bit seam (mimo_qam_softbits) on the GPU: the device function the trial kernel's soft
instances bin (csrc/softbits.h soft_axis, the closed form from the Gray code's pattern) against the
brute-force reference (tests/soft_ref.py), bit for bit, for every constellation size -- on the grid
x, y in {k / 8} over [-L - 2, L + 2], which holds every level, every midpoint between levels and
points beyond the outer levels, and on random doubles."""
import numpy as np
import pytest

import _engine
import soft_ref

pytestmark = pytest.mark.gpu

SIZES = [4, 16, 64, 256, 1024, 4096]


def assert_same_bits(got, want, label):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{label}: {len(bad)} values differ, first {bad[:3].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("M", SIZES)
def test_softbits_on_the_eighth_grid(M):
    """Every point of the grid x, y in {k / 8} over [-L - 2, L + 2] (1,057^2 points at M 4096) through
    the seam.  The metric of an axis reads that axis' coordinate alone, so the reference is the
    brute-force lambda of the grid's values, once, laid out over the grid."""
    L = int(round(np.sqrt(M)))
    hb = L.bit_length() - 1
    g = np.arange(-8 * (L + 2), 8 * (L + 2) + 1) / 8.0
    n = g.size
    z = (g[:, None] + 1j * g[None, :]).reshape(-1)
    axis = soft_ref.axis_lambda(M, g)                      # [n, hb]
    want = np.empty((n, n, 2 * hb))
    want[:, :, :hb] = axis[:, None, :]                     # the I-axis bits follow x
    want[:, :, hb:] = axis[None, :, :]                     # the Q-axis bits follow y
    got = _engine.qam_softbits(M, z)
    assert got.shape == (n * n, 2 * hb)
    assert_same_bits(got, want.reshape(n * n, 2 * hb), f"M={M} grid")
    # the layout against the whole-point reference on one row and one column of the grid
    for sub in (z[:n], z[::n]):
        assert_same_bits(_engine.qam_softbits(M, sub), soft_ref.lam(M, sub), f"M={M} grid line")
    # a midpoint between two levels is the decision boundary of one bit: lambda exactly 0 there
    mid = np.arange(-L + 2, L - 1, 2.0)
    if mid.size:
        assert np.all((_engine.qam_softbits(M, mid + 0j)[:, :hb] == 0).sum(axis=1) == 1)


@pytest.mark.parametrize("M", SIZES)
def test_softbits_on_random_doubles(M):
    L = int(round(np.sqrt(M)))
    rng = np.random.default_rng(M + 1)
    z = rng.uniform(-L - 2, L + 2, 4096) + 1j * rng.uniform(-L - 2, L + 2, 4096)
    # ... with the doubles next to every midpoint and level among them, where a rounded index picks the neighbour
    edge = np.arange(-L - 1, L + 2, dtype=np.float64)
    z[:edge.size] = np.nextafter(edge, np.inf) + 1j * np.nextafter(edge, -np.inf)
    assert_same_bits(_engine.qam_softbits(M, z), soft_ref.lam(M, z), f"M={M} random")


def test_softbits_size_rules():
    assert _engine.qam_softbits(16, np.zeros(0, np.complex128)).shape == (0, 4)
    for bad in (8, 2, 16384):
        with pytest.raises(_engine.EngineError, match="square QAM"):
            _engine.qam_softbits(bad, np.zeros(4, np.complex128))
