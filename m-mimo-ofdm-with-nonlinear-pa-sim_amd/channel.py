"""Frequency-domain MISO channels (reference channel.py), MI355X build.

Same classes and call signatures.  ``propagate`` (sum over antennas of H * Y) runs on the
GPU.  Channel matrices are closed-form geometry (LoS / two-path) or PCG64 draws
(Rayleigh, reference semantics) computed on the host when a caller asks for them; the
Link hot path does not use them -- it regenerates the per-trial channel on the device.
QuaDRiGa / random-paths channels need MATLAB or a NumPy-1 API and are out of scope;
``MisoTdlFd`` is the frequency-selective channel in their place (a tapped-delay-line profile), and
``MisoRaysFd`` the sum of paths ``MisoRandomPathsFd`` stands for: taps that are sums of rays.
"""
from __future__ import annotations

import numpy as np
from numpy import ndarray

import _engine
import utilities

SPEED_OF_LIGHT = 299792458.0  # scipy.constants.c


def carrier_freqs(n_fft: int, carrier_spacing, center_freq) -> ndarray:
    """``torch.fft.fftfreq(n_fft, d=1/n_fft).numpy() * df + fc`` (channel.py:52-53).

    torch's fftfreq is float32 and the Python-int operands keep the result float32, so the
    reference's carrier grid is float32-quantised; mirrored exactly (float64 output).
    """
    k = np.fft.fftfreq(n_fft, d=1 / n_fft).astype(np.float32)
    return (k * np.float32(carrier_spacing) + np.float32(center_freq)).astype(np.float64)


def _distances(tx_transceivers, rx_transceiver):
    tx = np.asarray([[t.cord_x, t.cord_y, t.cord_z] for t in tx_transceivers], dtype=np.float64)
    rx = np.asarray([rx_transceiver.cord_x, rx_transceiver.cord_y, rx_transceiver.cord_z], dtype=np.float64)
    return tx, rx, np.sqrt(np.sum((tx - rx) ** 2, axis=1))


def _propagate(channel_mat_fd, in_sig_mat, sum_signals):
    if sum_signals:
        h = np.asarray(channel_mat_fd, np.complex128)
        y = np.broadcast_to(np.asarray(in_sig_mat, np.complex128), h.shape)
        return _engine.combine(h, y)
    return np.multiply(in_sig_mat, channel_mat_fd)


class MisoLosFd:
    """(channel.py:11-89)"""

    def __init__(self):
        self.channel_mat_fd = None

    def __str__(self):
        return "los"

    def get_channel_mat_fd(self) -> ndarray:
        return self.channel_mat_fd

    def calc_channel_mat(self, tx_transceivers, rx_transceiver, skip_attenuation: bool = False) -> None:
        f = carrier_freqs(rx_transceiver.modem.n_fft, rx_transceiver.carrier_spacing, rx_transceiver.center_freq)
        _, _, d = _distances(tx_transceivers, rx_transceiver)
        gains = np.asarray([t.tx_ant_gain_db for t in tx_transceivers], dtype=np.float64)
        ph = np.exp(2j * np.pi * np.outer(d, f) / SPEED_OF_LIGHT)
        if skip_attenuation:
            self.channel_mat_fd = ph
        else:
            att = np.sqrt(np.power(10, (gains[:, None] + rx_transceiver.rx_ant_gain_db) / 10)) * \
                (SPEED_OF_LIGHT / (4 * np.pi * np.outer(d, f)))
            self.channel_mat_fd = ph * att

    def propagate(self, in_sig_mat: ndarray, sum_signals: bool = True) -> ndarray:
        return _propagate(self.channel_mat_fd, in_sig_mat, sum_signals)


class MisoTwoPathFd:
    """(channel.py:92-184): LoS + ground reflection with coefficient -1."""

    def __init__(self):
        self.channel_mat_fd = None

    def __str__(self):
        return "two_path"

    def get_channel_mat_fd(self) -> ndarray:
        return self.channel_mat_fd

    def calc_channel_mat(self, tx_transceivers, rx_transceiver, skip_attenuation: bool = False) -> None:
        f = carrier_freqs(rx_transceiver.modem.n_fft, rx_transceiver.carrier_spacing, rx_transceiver.center_freq)
        tx, rx, d_los = _distances(tx_transceivers, rx_transceiver)
        gains = np.asarray([t.tx_ant_gain_db for t in tx_transceivers], dtype=np.float64)
        horiz = np.sqrt((tx[:, 0] - rx[0]) ** 2 + (tx[:, 1] - rx[1]) ** 2)
        elev = np.arctan((tx[:, 2] + rx[2]) / horiz)
        d_sec = tx[:, 2] / np.sin(elev) + rx[2] / np.sin(elev)
        los = np.exp(2j * np.pi * np.outer(d_los, f) / SPEED_OF_LIGHT)
        sec = -1.0 * np.exp(2j * np.pi * np.outer(d_sec, f) / SPEED_OF_LIGHT)
        if not skip_attenuation:
            g = np.sqrt(np.power(10, (gains[:, None] + rx_transceiver.rx_ant_gain_db) / 10))
            los = los * g * (SPEED_OF_LIGHT / (4 * np.pi * np.outer(d_los, f)))
            sec = sec * g * (SPEED_OF_LIGHT / (4 * np.pi * np.outer(d_sec, f)))
        self.channel_mat_fd = los + sec

    def propagate(self, in_sig_mat: ndarray, sum_signals: bool = True) -> ndarray:
        return _propagate(self.channel_mat_fd, in_sig_mat, sum_signals)


class MisoRayleighFd:
    """(channel.py:187-292): i.i.d. CN(0,1) x free-space attenuation."""

    def __init__(self, tx_transceivers, rx_transceiver, seed: int = None):
        self.n_inputs = len(tx_transceivers)
        self.fd_samp_size = tx_transceivers[0].modem.n_fft
        self.seed = 1234 if seed is None else seed
        self.rng_gen = np.random.default_rng(self.seed)
        f = carrier_freqs(rx_transceiver.modem.n_fft, rx_transceiver.carrier_spacing, rx_transceiver.center_freq)
        _, _, d = _distances(tx_transceivers, rx_transceiver)
        gains = np.asarray([t.tx_ant_gain_db for t in tx_transceivers], dtype=np.float64)
        self.los_fd_att_mat = np.sqrt(np.power(10, (gains[:, None] + rx_transceiver.rx_ant_gain_db) / 10)) * \
            (SPEED_OF_LIGHT / (4 * np.pi * np.outer(d, f)))
        self.fd_att_mat = None
        self.set_channel_mat_fd()

    def __str__(self):
        return "rayleigh"

    def set_channel_mat_fd(self, channel_mat_fd: ndarray = None, skip_attenuation: bool = False) -> None:
        if channel_mat_fd is None:
            self.reroll_channel_coeffs(skip_attenuation)
        else:
            self.channel_mat_fd = channel_mat_fd

    def get_channel_mat_fd(self) -> ndarray:
        return self.channel_mat_fd

    def reroll_channel_coeffs(self, skip_attenuation: bool = False) -> None:
        c = self.rng_gen.standard_normal(size=(self.n_inputs, self.fd_samp_size * 2)).view(
            dtype=np.complex128) / np.sqrt(2.0)
        self.channel_mat_fd = c if skip_attenuation else np.multiply(c, self.los_fd_att_mat)

    def propagate(self, in_sig_mat: ndarray, sum_signals: bool = True) -> ndarray:
        return _propagate(self.channel_mat_fd, in_sig_mat, sum_signals)


class MisoTdlFd:
    """Tapped-delay-line Rayleigh channel: a frequency-selective stand-in for the reference's
    ``MisoRandomPathsFd`` / ``MisoQuadrigaFd`` (out of scope) with the reference classes' surface.

    Every antenna has ``len(delays)`` independent complex-normal taps at whole-sample ``delays``
    (strictly ascending, ``0 <= d < n_fft``) with mean powers ``10 ** (powers_db / 10)``, used as
    given (``utilities.exp_pdp`` returns a normalised profile), and
    ``H[a, n] = sum_l g[a, l] exp(-2j pi n delays[l] / n_fft)`` in numpy.fft bin order
    (``include/mimo_engine.h``, mimo_tdl).  ``ant_amp`` is ``MisoRayleighFd``'s per-antenna
    attenuation (antenna gains and free-space loss over the antenna's distance) taken at the
    centre frequency, bin 0 of the carrier grid: one amplitude per antenna, where the Rayleigh
    class has one per antenna and sub-carrier.

    The realisations come from the engine's own generator through the fine seam
    (``_engine.tdl_channels``): realisation ``i`` of this object is trial ``i`` under the key
    ``seed``.  ``Link.simulate(reroll_chan=True)`` draws its per-trial channels on the device from
    the same profile under the run's own seeds."""

    def __init__(self, tx_transceivers, rx_transceiver, delays, powers_db, seed: int = None):
        self.n_inputs = len(tx_transceivers)
        self.fd_samp_size = tx_transceivers[0].modem.n_fft
        self.seed = 1234 if seed is None else seed
        d = np.asarray(delays)
        p_db = np.asarray(powers_db, dtype=np.float64)
        if d.ndim != 1 or p_db.shape != d.shape:
            raise ValueError("delays and powers_db must be one-dimensional and of equal length")
        if not 1 <= d.size <= _engine.TDL_MAX_TAPS:
            raise ValueError(f"the profile must have 1 ... {_engine.TDL_MAX_TAPS} taps")
        if np.any(d != np.floor(d)):
            raise ValueError("delays must be whole samples")
        if d[0] < 0 or d[-1] >= self.fd_samp_size or np.any(np.diff(d) <= 0):
            raise ValueError("delays must be strictly ascending in [0, n_fft)")
        if not np.all(np.isfinite(p_db)):
            raise ValueError("powers_db must be finite")
        self.delays = d.astype(np.int32)
        self.powers = np.power(10.0, p_db / 10)
        f = carrier_freqs(rx_transceiver.modem.n_fft, rx_transceiver.carrier_spacing, rx_transceiver.center_freq)
        _, _, dist = _distances(tx_transceivers, rx_transceiver)
        gains = np.asarray([t.tx_ant_gain_db for t in tx_transceivers], dtype=np.float64)
        self.ant_amp = np.sqrt(np.power(10, (gains + rx_transceiver.rx_ant_gain_db) / 10)) * \
            (SPEED_OF_LIGHT / (4 * np.pi * dist * f[0]))
        self.n_drawn = 0  # realisations drawn so far: the trial index of the next one
        self.channel_mat_fd = None
        self.set_channel_mat_fd()

    def __str__(self):
        return "tdl"

    def set_channel_mat_fd(self, channel_mat_fd: ndarray = None, skip_attenuation: bool = False) -> None:
        if channel_mat_fd is None:
            self.reroll_channel_coeffs(skip_attenuation)
        else:
            self.channel_mat_fd = channel_mat_fd

    def get_channel_mat_fd(self) -> ndarray:
        return self.channel_mat_fd

    def reroll_channel_coeffs(self, skip_attenuation: bool = False) -> None:
        self.channel_mat_fd = _engine.tdl_channels(self.delays, self.powers, self.n_inputs, self.fd_samp_size,
                                                   self.seed, self.n_drawn, 1,
                                                   ant_amp=None if skip_attenuation else self.ant_amp)[0]
        self.n_drawn += 1

    def propagate(self, in_sig_mat: ndarray, sum_signals: bool = True) -> ndarray:
        return _propagate(self.channel_mat_fd, in_sig_mat, sum_signals)


class MisoRaysFd:
    """Ray-cluster channel: ``MisoTdlFd`` with every tap a sum of rays towards point scatterers, so
    that the taps are correlated over the array (``include/mimo_engine.h``, mimo_rays) -- what the
    reference's ``MisoRandomPathsFd`` stands for, with the reference classes' surface.

    Ray ``r`` belongs to tap ``ray_tap[r]`` (non-decreasing from 0 in steps of 0 or 1) at the
    whole-sample delay ``delays[ray_tap[r]]``, points at ``points[r]`` [R, 3] and has amplitude
    ``ray_amp[r]``; ``ray_kind[r]`` is 0 for a diffuse ray (a complex-normal gain per realisation) or
    1 for a specular one (unit modulus, uniform phase).  Its steering vector is
    ``utilities.scatterer_steering`` at the centre frequency, bin 0 of the carrier grid, times
    ``MisoTdlFd``'s per-antenna ``ant_amp``; ``skip_attenuation`` leaves that amplitude out.
    ``utilities.ring_clusters`` makes a stand-in geometry.

    The realisations come from the engine's own generator through the fine seam
    (``_engine.rays_channels``): realisation ``i`` of this object is trial ``i`` under the key
    ``seed``.  ``Link.simulate(reroll_chan=True)`` draws its per-trial channels on the device from the
    same profile under the run's own seeds."""

    def __init__(self, tx_transceivers, rx_transceiver, delays, ray_tap, ray_amp, points, ray_kind=None,
                 seed: int = None):
        self.n_inputs = len(tx_transceivers)
        self.fd_samp_size = tx_transceivers[0].modem.n_fft
        self.seed = 1234 if seed is None else seed
        d, rt = np.asarray(delays), np.asarray(ray_tap)
        amp, pts = np.asarray(ray_amp, dtype=np.float64), np.asarray(points, dtype=np.float64)
        if d.ndim != 1 or not 1 <= d.size <= _engine.TDL_MAX_TAPS:
            raise ValueError(f"the profile must have 1 ... {_engine.TDL_MAX_TAPS} taps")
        if np.any(d != np.floor(d)):
            raise ValueError("delays must be whole samples")
        if d[0] < 0 or d[-1] >= self.fd_samp_size or np.any(np.diff(d) <= 0):
            raise ValueError("delays must be strictly ascending in [0, n_fft)")
        if rt.ndim != 1 or not d.size <= rt.size <= _engine.RAYS_MAX:
            raise ValueError(f"the profile must have n_taps ... {_engine.RAYS_MAX} rays")
        if np.any(rt != np.floor(rt)) or rt[0] != 0 or rt[-1] != d.size - 1 or not np.all(np.isin(np.diff(rt), (0, 1))):
            raise ValueError("ray_tap must be non-decreasing from 0 to n_taps - 1 in steps of 0 or 1")
        if amp.shape != rt.shape or not np.all(np.isfinite(amp)) or np.any(amp <= 0):
            raise ValueError("ray_amp must hold one finite amplitude > 0 per ray")
        if pts.shape != (rt.size, 3) or not np.all(np.isfinite(pts)):
            raise ValueError("points must be [n_rays, 3] and finite")
        if ray_kind is None:
            kind = np.zeros(rt.size, np.uint8)
        else:
            kind = np.asarray(ray_kind)
            if kind.shape != rt.shape or not np.all(np.isin(kind, (0, 1))):
                raise ValueError("ray_kind must hold 0 (diffuse) or 1 (specular) per ray")
        self.delays = d.astype(np.int32)
        self.ray_tap = rt.astype(np.int32)
        self.ray_amp = amp
        self.ray_kind = kind.astype(np.uint8)
        self.points = pts
        f = carrier_freqs(rx_transceiver.modem.n_fft, rx_transceiver.carrier_spacing, rx_transceiver.center_freq)
        tx, _, dist = _distances(tx_transceivers, rx_transceiver)
        gains = np.asarray([t.tx_ant_gain_db for t in tx_transceivers], dtype=np.float64)
        self.ant_amp = np.sqrt(np.power(10, (gains + rx_transceiver.rx_ant_gain_db) / 10)) * \
            (SPEED_OF_LIGHT / (4 * np.pi * dist * f[0]))
        self.steer_phase = utilities.scatterer_steering(tx, pts, f[0])  # [A, R], unit modulus
        self.n_drawn = 0  # realisations drawn so far: the trial index of the next one
        self.channel_mat_fd = None
        self.set_channel_mat_fd()

    def __str__(self):
        return "rays"

    def steer(self, skip_attenuation: bool = False) -> ndarray:
        """The rays' steering vectors [A, R]: the phases, times ``ant_amp`` unless skipped."""
        return self.steer_phase if skip_attenuation else self.steer_phase * self.ant_amp[:, None]

    def set_channel_mat_fd(self, channel_mat_fd: ndarray = None, skip_attenuation: bool = False) -> None:
        if channel_mat_fd is None:
            self.reroll_channel_coeffs(skip_attenuation)
        else:
            self.channel_mat_fd = channel_mat_fd

    def get_channel_mat_fd(self) -> ndarray:
        return self.channel_mat_fd

    def reroll_channel_coeffs(self, skip_attenuation: bool = False) -> None:
        self.channel_mat_fd = _engine.rays_channels(self.delays, self.ray_tap, self.ray_amp, self.steer(skip_attenuation),
                                                    self.fd_samp_size, self.seed, self.n_drawn, 1,
                                                    ray_kind=self.ray_kind)[0]
        self.n_drawn += 1

    def propagate(self, in_sig_mat: ndarray, sum_signals: bool = True) -> ndarray:
        return _propagate(self.channel_mat_fd, in_sig_mat, sum_signals)
