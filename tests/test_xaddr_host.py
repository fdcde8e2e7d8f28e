"""Host mirror of the transform addresses that the float64 wave-split instances hold across the antenna
loop (csrc/tuning.h MIMO_XADDR, MIMO_XADDR_TW; csrc/wave_fft.h XAddr): mimo_probe_xaddr packs every
thread's words with the kernel's own constexpr formulas and unpacks them with the kernel's accessors.

For both team shapes (T 128 / F 1024: two waves, NB = 4; T 256 / F 2048: four waves, NB = 2), every
thread t < T and every use site, the unpacked byte offset
  * equals the formula the transforms derive from the thread id where the switch is off, restated
    here from csrc/wave_fft.h run / run_second and csrc/team_fft.h stage / butterfly;
  * with each immediate offset of its use stays inside the structure it addresses: the wave's
    exchange row (the cross-wave step: the row's first FW cells; the transposed exchange 0: the
    F / R0 payload cells of a transposed row; exchange 1: the padded cells of elements < FW), the
    stage's block of the LDS constants, the F inter-step entries of the twiddle table;
  * is 16-byte aligned and below 65,536 (it is held in 16 bits).
Each exchange's writes and reads also cover the same cells once each.  The check fails when any half
of any thread's words is moved by one element or by half an element."""
import ctypes

import numpy as np
import pytest

import probe_util

SHAPES = {1024: (128, 2, 4), 2048: (256, 4, 2)}  # F: T, waves, NB
INFO = ("T", "WV", "P", "NB", "FW", "ROW", "LDS", "R0", "XS0", "NS1", "NS2", "CT1", "CT2", "TWL_N", "TW_INTER", "CB",
        "Q1", "Q2", "PSH1", "TABLE", "CT")
N_SITES = 10
HALVES = [(word, shift) for word in range(3) for shift in (0, 16)]


def _probe(F, words_in=None):
    T = SHAPES[F][0]
    fn = probe_util.lib().mimo_probe_xaddr
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_int32] + [ctypes.c_void_p] * 4
    words = np.zeros((T, 3), np.uint32)
    sites = np.zeros((T, N_SITES), np.uint32)
    info = np.zeros(len(INFO), np.int32)
    win = None if words_in is None else np.ascontiguousarray(words_in, np.uint32).ctypes.data
    probe_util._check(fn(F, win, words.ctypes.data, sites.ctypes.data, info.ctypes.data))
    return words, sites.astype(np.int64), dict(zip(INFO, info.tolist()))


def _problems(F, words, sites, k):
    """Every way the unpacked offsets of one shape miss the three properties (empty: none)."""
    T, P, NB, WV, ROW, FW, E = k["T"], k["P"], k["NB"], k["WV"], k["ROW"], k["FW"], k["CB"]
    R0, XS0, NS1, NS2 = k["R0"], k["XS0"], k["NS1"], k["NS2"]
    R1 = NS2 // NS1
    t = np.arange(T)
    w, l = t >> 6, t & 63
    pad = lambda e: e + (e >> k["PSH1"])
    out = []

    def need(ok, what):
        if not np.all(ok):
            out.append(what)

    want = {
        0: E * t,                                                   # lds[row_of(k1) + t + T i]
        1: E * (w * ROW + l),                                       # lds + row_of(w) + l
        2: E * (w * ROW + (l % R0) * XS0 + l // R0),                # buf + (t % R0) XS0 + t / R0
        3: E * (w * ROW + pad((l // NS1) * NS1 * R1 + (l & (NS1 - 1)))),  # buf + pad((j / NS) NS R + jm)
        4: E * (w * ROW + pad(l)),                                  # buf + pad(t)
        5: E * (l & (NS1 - 1)),                                     # tw1 + ct_off(1) + (t & (NS - 1))
        6: E * (l & (NS2 - 1)),
        7: E * t,                                                   # entry k n2, n2 = t + T i
        8: E * 2 * t,
        9: E * w * l,                                               # entry w (l + 64 m)
    }
    for s, v in want.items():
        need(sites[:, s] == v, f"site {s}: not the thread-id formula")
    # the halves themselves, low half first: cross | row, x0r | x1w, tw | x1r
    halves = np.stack([words & 0xFFFF, words >> 16], axis=2).reshape(T, 6).astype(np.int64)
    for h, s in enumerate((0, 1, 2, 3, None, 4)):
        need(halves[:, h] == (E * l if s is None else want[s]), f"half {h}: not the thread-id formula")
    need(halves % 16 == 0, "alignment of the halves")
    need(sites % 16 == 0, "alignment")
    need((sites >= 0) & (sites < 65536), "16-bit range")

    elem = sites // E  # whole elements from here on (alignment is checked above)
    row0 = (w * ROW)[:, None]
    # cross-wave step: cell [row k1][t + T i], both transforms
    for k1 in range(WV):
        c = elem[:, 0:1] + k1 * ROW + T * np.arange(NB)[None, :]
        need((c >= k1 * ROW) & (c < k1 * ROW + FW), f"cross-wave cells of row {k1}")
    # ... and the wave's own row [row w][l + 64 m]
    c = elem[:, 1:2] + 64 * np.arange(P)[None, :]
    need((c >= row0) & (c < row0 + FW), "own-row cells")
    for wave in range(WV):
        mine = w == wave
        cells = np.sort(c[mine].ravel())
        need(np.array_equal(cells, wave * ROW + np.arange(FW)) if cells.size == FW else False, "own-row cover")
        # transposed exchange 0: stage 0 writes [r][l] at row + r XS0, stage 1 reads (t % R0) XS0 + t / R0 + (64 / R0) m
        wr = elem[mine, 1:2] + XS0 * np.arange(R0)[None, :]
        rd = elem[mine, 2:3] + (64 // R0) * np.arange(P)[None, :]
        need((wr >= wave * ROW) & (wr < (wave + 1) * ROW), "exchange 0 writes in the row")
        need(((rd - wave * ROW) % XS0 < FW // R0) & (rd >= wave * ROW) & (rd < wave * ROW + R0 * XS0),
             "exchange 0 reads in a transposed row's payload")
        need(np.array_equal(np.sort(wr.ravel()), np.sort(rd.ravel())) and np.unique(wr).size == FW, "exchange 0 cover")
        # exchange 1: stage 1 writes pad(base + r NS1), stage 2 reads pad(l + 64 m)
        wr = elem[mine, 3:4] + pad(NS1 * np.arange(R1))[None, :]
        rd = elem[mine, 4:5] + pad(64 * np.arange(P))[None, :]
        cells = wave * ROW + pad(np.arange(FW))
        need(np.array_equal(np.sort(wr.ravel()), cells), "exchange 1 writes")
        need(np.array_equal(np.sort(rd.ravel()), cells), "exchange 1 reads")
        need(cells.max() < (wave + 1) * ROW, "exchange 1 in the row")
    need(k["LDS"] == WV * ROW and E * k["LDS"] <= 65536, "exchange array")
    # stage constants: rows [Q][NS] of stage 1 at CT1 and stage 2 at CT2 of the LDS copy; without the
    # cot-tan form stage 2's rows are its block of the table in global memory, ahead of TW_INTER
    for s, off, q, ns in ((5, k["CT1"], k["Q1"], NS1), (6, k["CT2"], k["Q2"], NS2)):
        c = elem[:, s:s + 1] + off + ns * np.arange(q)[None, :]
        end = k["TWL_N"] if (k["CT"] or s == 5) else k["TW_INTER"]
        need((c >= off) & (c < off + q * ns) & (c < end), f"stage constants, site {s}")
        need(elem[:, s] < ns, f"stage constants' lane, site {s}")
    # inter-step twiddles: F entries from TW_INTER, exp(-j 2 pi n / F)
    for s, kk in ((7, 1), (8, 2)):
        if kk < WV:
            n = elem[:, s:s + 1] + kk * T * np.arange(NB)[None, :]
            need((n >= 0) & (n < F), f"inverse twiddle entries, k = {kk}")
            need(n == kk * (t[:, None] + T * np.arange(NB)[None, :]), f"inverse twiddle index, k = {kk}")
    n = elem[:, 9:10] + 64 * w[:, None] * np.arange(P)[None, :]
    need((n >= 0) & (n < F), "forward twiddle entries")
    need(k["TW_INTER"] + F <= k["TABLE"], "twiddle table")
    return out


@pytest.mark.parametrize("F", list(SHAPES))
def test_layout_is_the_one_the_formulas_assume(F):
    _, _, k = _probe(F)
    T, WV, NB = SHAPES[F]
    assert (k["T"], k["WV"], k["NB"], k["P"], k["FW"], k["CB"]) == (T, WV, NB, 8, 512, 16)
    assert (k["R0"], k["XS0"], k["ROW"], k["NS1"], k["NS2"], k["PSH1"]) == (8, 68, 544, 8, 64, 5)
    assert k["CT"] == (1 if F == 2048 else 0)  # the two-wave team keeps stage twiddles (no LDS room for stage 2's rows)


@pytest.mark.parametrize("F", list(SHAPES))
def test_unpacked_addresses(F):
    words, sites, k = _probe(F)
    assert _problems(F, words, sites, k) == []
    # the halves as documented: low half first
    np.testing.assert_array_equal(words[:, 0], sites[:, 0] | sites[:, 1] << 16)
    np.testing.assert_array_equal(words[:, 1], sites[:, 2] | sites[:, 3] << 16)
    np.testing.assert_array_equal(words[:, 2], sites[:, 6] | sites[:, 4] << 16)
    # words handed in come back through the same accessors
    again = _probe(F, words)
    np.testing.assert_array_equal(again[0], words)
    np.testing.assert_array_equal(again[1], sites)


@pytest.mark.parametrize("F", list(SHAPES))
@pytest.mark.parametrize("delta", [16, 8])
def test_any_perturbed_half_fails(F, delta):
    words, _, k = _probe(F)
    T = k["T"]
    for word, shift in HALVES:
        # one probe call per half: thread t's half moved in copy t (each copy checked on its own)
        missed = []
        for t in range(0, T, 1):
            bad = words.copy()
            half = (int(bad[t, word]) >> shift) & 0xFFFF
            moved = (half + delta) & 0xFFFF
            bad[t, word] = (int(bad[t, word]) & ~(0xFFFF << shift) & 0xFFFFFFFF) | (moved << shift)
            back, sites, _ = _probe(F, bad)
            if not _problems(F, back, sites, k):
                missed.append(t)
        assert missed == [], f"word {word} shift {shift}: unnoticed at threads {missed}"
