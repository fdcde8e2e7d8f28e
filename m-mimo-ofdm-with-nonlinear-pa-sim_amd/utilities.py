"""Numeric utilities of the reference (utilities.py), MI355X build.

Array compute (FFTs, bit-error counts) runs on the GPU through the C ABI; bit packing,
dB conversions, geometry helpers and CSV I/O are host-side format work.
Plotting helpers of the reference are out of scope.
"""
from __future__ import annotations

import csv

import numpy as np
from numpy import ndarray

import _engine


def dec2bitarray(in_number, bit_width: int) -> ndarray:
    """MSB-first bits of an int or int array (utilities.py:18-32)."""
    if isinstance(in_number, (np.integer, int)):
        return decimal2bitarray(int(in_number), bit_width).copy()
    nums = np.asarray(in_number, dtype=np.int64).reshape(-1)
    shifts = np.arange(bit_width - 1, -1, -1)
    return ((nums[:, None] >> shifts[None, :]) & 1).astype(np.int8).reshape(-1)


def decimal2bitarray(number: int, bit_width: int) -> ndarray:
    """(utilities.py:35-51)"""
    shifts = np.arange(bit_width - 1, -1, -1)
    return ((int(number) >> shifts) & 1).astype(np.int8)


def bitarray2dec(in_bitarray: ndarray) -> int:
    """(utilities.py:54-67)"""
    b = np.asarray(in_bitarray, dtype=np.int64).reshape(-1)
    return int((b * (1 << np.arange(b.size - 1, -1, -1))).sum()) if b.size else 0


def td_signal_power(signal: ndarray) -> float:
    """(utilities.py:70-79)"""
    return float(np.mean(np.abs(signal) ** 2))


def fd_signal_power(signal: ndarray) -> float:
    """(utilities.py:82-91)"""
    return float(np.sum(np.abs(signal) ** 2))


def count_mismatched_bits(tx_bits_arr: ndarray, rx_bits_arr: ndarray) -> int:
    """sum(tx XOR rx) on the GPU (utilities.py:94-104)."""
    return _engine.count_bit_errors(tx_bits_arr, rx_bits_arr)


def ebn0_to_snr(eb_per_n0, n_fft: int, n_sub_carr: int, constel_size: int):
    """(utilities.py:107-118)"""
    return 10 * np.log10(10 ** (np.asarray(eb_per_n0) / 10) * n_sub_carr * np.log2(constel_size) / n_fft)


def snr_to_ebn0(snr, n_fft: int, n_sub_carr: int, constel_size: int):
    """(utilities.py:121-133)"""
    return 10 * np.log10(10 ** (np.asarray(snr) / 10) * (n_fft / (n_sub_carr * np.log2(constel_size))))


def to_db(samples):
    """(utilities.py:136-143)"""
    return 10 * np.log10(samples)


def pts_on_circum(radius: float, n_points: int = 100) -> list:
    """(utilities.py:146-155)"""
    return [(np.cos(2 * np.pi / n_points * x) * radius, np.sin(2 * np.pi / n_points * x) * radius)
            for x in range(0, n_points + 1)]


def pts_on_semicircum(radius: float, n_points: int = 100) -> list:
    """(utilities.py:158-167)"""
    return [(np.cos(np.pi / n_points * x) * radius, np.sin(np.pi / n_points * x) * radius)
            for x in range(0, n_points + 1)]


def circle_probes(angles_deg, radius: float, z: float = 0.0) -> ndarray:
    """Probe positions ``(r cos theta, r sin theta, z)`` [m] on the horizontal circle of ``radius``
    around the origin at height ``z``, one row per angle [deg]: the ``probes`` of
    ``Link.beampattern``."""
    th = np.deg2rad(np.asarray(angles_deg, dtype=np.float64).reshape(-1))
    return np.stack([radius * np.cos(th), radius * np.sin(th), np.full(th.shape, float(z))], axis=1)


def pts_on_semisphere(radius: float, n_points: int = 100, center_x: float = 0, center_y: float = 0,
                      center_z: float = 0):
    """(utilities.py:170-192)"""
    az = np.deg2rad(np.linspace(0, 180, int(np.sqrt(n_points)), endpoint=True))
    el = np.deg2rad(np.linspace(0, 180, int(np.sqrt(n_points)), endpoint=True))
    pts = []
    for a in az:
        for e in el:
            pts.append((-radius * np.sin(e) * np.cos(a) + center_x, -radius * np.sin(e) * np.sin(a) + center_y,
                        -radius * np.cos(e) + center_z))
    return pts


def to_freq_domain(in_sig_td: ndarray, remove_cp: bool = True, cp_len: int = None) -> ndarray:
    """Drop CP, ortho FFT along the last axis, on the GPU (utilities.py:311-329)."""
    x = np.asarray(in_sig_td)
    if remove_cp:
        x = x[..., cp_len:]
    return _engine.fft(x, inverse=False)


def to_time_domain(in_sig_mat_fd: ndarray) -> ndarray:
    """Ortho IFFT along the last axis, on the GPU (utilities.py:332-339)."""
    return _engine.fft(np.asarray(in_sig_mat_fd), inverse=True)


def qc_ldpc_code(z: int, n_rows: int, n_cols: int, n_dec_iters: int = 10, seed: int = 0):
    """A deterministic QC-LDPC code for the coded mode (``_engine.LdpcCode``): lifting size ``z``, a
    base matrix of ``n_rows`` x ``n_cols`` blocks, every block a shifted identity (none empty), and no
    4-cycles.  With ``g = np.random.default_rng(seed)``, column by column ``g.integers(0, z, n_rows)``
    is drawn up to 1,000 times and the first draw is kept for which
    ``(s[r1, c0] - col[r1] + col[r2] - s[r2, c0]) % z != 0`` for every earlier column ``c0`` and every
    pair of rows ``r1 < r2``; ``ValueError`` if none is.  No standard's table: a stand-in of the same
    structure for anyone who has none at hand."""
    z, n_rows, n_cols = int(z), int(n_rows), int(n_cols)
    g = np.random.default_rng(seed)
    s = np.zeros((n_rows, n_cols), dtype=np.int64)
    r1, r2 = np.triu_indices(n_rows, 1)
    for c in range(n_cols):
        for _ in range(1000):
            col = g.integers(0, z, n_rows)
            d = (s[r1, :c] - col[r1, None] + col[r2, None] - s[r2, :c]) % z
            if np.all(d != 0):
                s[:, c] = col
                break
        else:
            raise ValueError(f"no 4-cycle-free column {c} for z {z}, {n_rows} x {n_cols} within 1,000 draws")
    return _engine.LdpcCode(z, s, n_dec_iters)


def exp_pdp(n_taps: int, step: int, decay_db_per_tap: float):
    """An exponential power-delay profile for the TDL channel (``channel.MisoTdlFd``,
    ``_engine.Engine.set_tdl``): ``n_taps`` taps ``step`` whole samples apart from delay 0, tap ``l``
    ``l * decay_db_per_tap`` dB below the first, the linear powers normalised to sum 1.
    -> (delays int32 [n_taps], powers float64 [n_taps]); ``10 * np.log10(powers)`` is ``MisoTdlFd``'s
    ``powers_db``.  No standard's table: a stand-in of the usual shape for anyone who has none at hand."""
    n_taps, step = int(n_taps), int(step)
    if n_taps < 1 or step < 1:
        raise ValueError("n_taps and step must be >= 1")
    if not np.isfinite(decay_db_per_tap) or decay_db_per_tap < 0:
        raise ValueError("decay_db_per_tap must be finite and >= 0")
    p = np.power(10.0, -float(decay_db_per_tap) * np.arange(n_taps) / 10)
    return (np.arange(n_taps) * step).astype(np.int32), p / np.sum(p)


def scatterer_steering(tx_pos, points, freq: float) -> ndarray:
    """Steering vectors of rays towards point scatterers (``channel.MisoRaysFd``,
    ``_engine.Engine.set_rays``): ``exp(+2j pi freq |p_a - q_r| / c)`` for the antenna positions
    ``tx_pos`` [A, 3] and the ``points`` [R, 3], as [A, R].  The phase convention is the LoS classes'
    (``channel.MisoLosFd``): a ray towards a point is what ``MisoLosFd(skip_attenuation=True)`` gives
    at ``freq`` for a receiver standing there."""
    p = np.asarray(tx_pos, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    d = np.sqrt(np.sum((p[:, None, :] - q[None, :, :]) ** 2, axis=2))
    return np.exp(2j * np.pi * (d * float(freq)) / 299792458.0)


def ring_clusters(delays, powers, az_deg, spread_deg: float, rays_per_cluster: int, radius: float, z: float = 0.0,
                  k_db: float = None, los_point=None):
    """A stand-in geometry for the ray-cluster channel: one cluster of ``M = rays_per_cluster`` point
    scatterers per tap on the horizontal circle of ``radius`` around the origin at height ``z``.
    Cluster ``l`` sits at the azimuths ``az_deg[l] + o_m``, ``o_m = spread_deg (2 m - (M - 1))
    sqrt(3 / (M^2 - 1))``: ``M`` equally spaced offsets within ``+-sqrt(3) spread_deg`` whose rms is
    ``spread_deg`` exactly (the uniform distribution of that rms as ``M`` grows; ``M = 1``: offset 0).
    Every ray of it is diffuse with amplitude ``sqrt(powers[l] / M)``.  With ``k_db`` (a Rician K
    factor [dB], ``K = 10^(k_db / 10)``) one specular ray towards ``los_point`` joins tap 0 with
    power ``K / (K + 1) sum(powers)`` and every diffuse power is scaled by ``1 / (K + 1)``: the total
    stays ``sum(powers)``.
    -> (ray_tap int32 [R], ray_amp [R], ray_kind uint8 [R], points [R, 3]), the specular ray first;
    ``scatterer_steering(tx_pos, points, freq)`` gives the rays' steering vectors.  ``delays`` only
    fixes the number of taps.  No standard's table: a stand-in for anyone who has none at hand."""
    n_taps, m = len(np.asarray(delays).reshape(-1)), int(rays_per_cluster)
    p = np.asarray(powers, dtype=np.float64).reshape(-1)
    az = np.asarray(az_deg, dtype=np.float64).reshape(-1)
    if n_taps < 1 or p.size != n_taps or az.size != n_taps:
        raise ValueError("delays, powers and az_deg must hold one value per tap")
    if m < 1:
        raise ValueError("rays_per_cluster must be >= 1")
    if not np.isfinite(spread_deg) or spread_deg < 0 or not radius > 0:
        raise ValueError("spread_deg must be finite and >= 0, radius > 0")
    if (k_db is None) != (los_point is None):
        raise ValueError("k_db and los_point go together")
    off = np.zeros(1) if m == 1 else float(spread_deg) * (2 * np.arange(m) - (m - 1)) * np.sqrt(3.0 / (m * m - 1))
    k = 0.0 if k_db is None else 10.0 ** (float(k_db) / 10)
    ray_tap = np.repeat(np.arange(n_taps), m)
    ray_amp = np.repeat(np.sqrt(p / (k + 1) / m), m)
    ray_kind = np.zeros(n_taps * m, np.uint8)
    points = circle_probes((az[:, None] + off[None, :]).reshape(-1), radius, z)
    if k_db is not None:
        ray_tap = np.concatenate(([0], ray_tap))
        ray_amp = np.concatenate(([np.sqrt(k / (k + 1) * p.sum())], ray_amp))
        ray_kind = np.concatenate((np.ones(1, np.uint8), ray_kind))
        points = np.concatenate((np.asarray(los_point, dtype=np.float64).reshape(1, 3), points))
    return ray_tap.astype(np.int32), ray_amp, ray_kind, points


def save_to_csv(data_lst: list, filename: str, directory: str = "figs/csv_results") -> None:
    """One row per vector, ``csv.writer.writerows`` (utilities.py:342-352); the reference
    writes to ``figs/csv_results`` relative to the working directory."""
    import os
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "%s.csv" % filename), "w", newline="") as f:
        csv.writer(f).writerows([list(np.asarray(row, dtype=np.float64).reshape(-1)) for row in data_lst])


def read_from_csv(filename: str, directory: str = "../figs/csv_results") -> list:
    """List of float rows, ``QUOTE_NONNUMERIC`` (utilities.py:355-365; the reference reads
    from ``../figs/csv_results``)."""
    import os
    with open(os.path.join(directory, "%s.csv" % filename), "r", newline="") as f:
        return list(csv.reader(f, quoting=csv.QUOTE_NONNUMERIC))


def print_progress_bar(iteration: int, total: int, prefix: str = "", suffix: str = "", decimals: int = 1,
                       length: int = 100, fill: str = "#", print_end: str = "\r") -> None:
    """(utilities.py:369-392)"""
    percent = ("{0:." + str(decimals) + "f}").format(100 * (iteration / float(total)))
    filled = int(length * iteration // total)
    print(f"\r{prefix} |{fill * filled + '-' * (length - filled)}| {percent}% {suffix}", end=print_end)
    if iteration == total:
        print()
