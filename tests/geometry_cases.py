"""An off-default geometry for the trial kernel's parity tests, its case table and the oracle
mutants that show what the table can tell apart.  No GPU.

Every other parity test runs the lambda/2 line array at 3.5 GHz and 15 kHz seen from 300 m, with
the user on x = y: there the per-antenna factor ``ant_rel[a] = d0 / d_a`` and the per-sub-carrier
factor ``f_rel[k] = fc / f_k`` that the kernel takes out of its loops are within a percent of 1,
and the reference's quirk that both jittered coordinates are drawn around ``rx_loc_x``
(``oracle/sim.py`` ``channel_inband``) cannot be told from y jittering around ``rx_pos[1]``.
``off_default`` is a spread-out array close to a user whose x differs from its y, on a band 60 %
of the centre frequency wide.

``CASES`` holds the smallest shapes that reach each variant of the channel code (templated on the
slot map, the channel kind and CSI); ``tests/test_geometry_cases.py`` pins the conditions that
make the table worth running (counters neither empty nor saturated, unequal antennas, a wide
band, every mutant visible), ``tests/test_gpu_geometry.py`` runs it on the device.
"""
import contextlib
import functools

import numpy as np

from oracle import refmath as rm
from oracle import sim

SEED = 1313
ITERS = (0, 1, 2)        # counters: clean + these
RX_POS = (12.0, 7.0, 1.5)
RX_LOC_VAR = 4.0
CENTER_FREQ = 100e6
BAND = 0.6               # n_fft carrier spacings span this share of the centre frequency


def sparse_positions(n):
    """[n, 3]: an array that is neither a line nor compact -- x = linspace(-20, 20), y = 3 for
    the odd indices and 0 for the even ones, z = linspace(5, 15); one antenna: (3, 0, 9)."""
    if n == 1:
        return np.array([[3.0, 0.0, 9.0]])
    y = np.where(np.arange(n) % 2 == 1, 3.0, 0.0)
    return np.stack([np.linspace(-20.0, 20.0, n), y, np.linspace(5.0, 15.0, n)], axis=1)


def only_array(n_ant, n_fft):
    """The sparse array near the user, on the default band (diagnosis: ``ant_rel`` alone)."""
    return dict(tx_pos=sparse_positions(n_ant), rx_pos=RX_POS, rx_loc_var=RX_LOC_VAR)


def only_band(n_ant, n_fft):
    """The default array and user on the wide band (diagnosis: ``f_rel`` alone)."""
    return dict(center_freq=CENTER_FREQ, carrier_spacing=BAND * CENTER_FREQ / n_fft,
                tx_pos=rm.ula_positions(n_ant, 3.5e9, 0.5, 15.0))


def off_default(n_ant, n_fft):
    """``SimConfig`` keywords of the tested geometry: with S = F / 2 the band spans fc / f_k from
    0.87 to 1.18 and every carrier stays positive."""
    return dict(tx_pos=sparse_positions(n_ant), rx_pos=RX_POS, rx_loc_var=RX_LOC_VAR, center_freq=CENTER_FREQ,
                carrier_spacing=BAND * CENTER_FREQ / n_fft)


# F,    S,    A, M,  channel,    receiver, csi_eps, pa,       p,   ibo,  trials
CASES = [
    (128, 64, 5, 16, "rayleigh", "cnc", None, "toi", 0.0, 12.0, 24),
    (256, 100, 5, 64, "los", "cnc", None, "softlim", 0.0, 2.0, 24),
    (256, 100, 5, 64, "two_path", "mcnc", None, "softlim", 0.0, 2.0, 24),
    (512, 256, 8, 64, "rayleigh", "cnc", None, "softlim", 0.0, 2.0, 24),
    (512, 256, 8, 64, "rayleigh", "cnc", 0.2, "softlim", 0.0, 2.0, 24),
    (512, 256, 8, 64, "los", "cnc", None, "rapp", 2.5, 2.0, 24),
    (512, 256, 8, 64, "two_path", "cnc", None, "softlim", 0.0, 2.0, 24),
    (1024, 512, 8, 16, "rayleigh", "mcnc", 0.2, "softlim", 0.0, 2.0, 12),
    (2048, 1024, 8, 64, "los", "mcnc", None, "softlim", 0.0, 2.0, 8),
    (2048, 1024, 8, 64, "two_path", "cnc", None, "softlim", 0.0, 2.0, 8),
    (2048, 1024, 8, 64, "rayleigh", "cnc", None, "rapp", 3.0, 2.0, 8),
    (4096, 2048, 8, 64, "rayleigh", "cnc", 0.1, "softlim", 0.0, 2.0, 6),
    (4096, 2048, 8, 64, "two_path", "mcnc", None, "softlim", 0.0, 2.0, 6),
    (8192, 4096, 4, 64, "los", "cnc", None, "softlim", 0.0, 2.0, 4),
    (8192, 4096, 4, 64, "rayleigh", "cnc", 0.2, "softlim", 0.0, 2.0, 4),
    (8192, 2048, 4, 64, "two_path", "cnc", None, "softlim", 0.0, 2.0, 4),
]
CASE_NUMBERS = list(range(1, len(CASES) + 1))
# Eb/N0 [dB] per case number where 14 dB misses a condition of tests/test_geometry_cases.py
EBN0 = {1: 9.0}


def case_id(num):
    F, S, A, M, channel, receiver, csi, pa, p, ibo, n = CASES[num - 1]
    return f"{num}-F{F}-S{S}-A{A}-{channel}-{receiver}" + ("" if csi is None else "-csi")


def case_config(num, geometry=off_default):
    """(SimConfig, trial ids) of case ``num`` (1-based, the table's numbering)."""
    F, S, A, M, channel, receiver, csi, pa, p, ibo, n = CASES[num - 1]
    snr = float(rm.ebn0_to_snr(EBN0.get(num, 14.0), F, S, M))
    cfg = sim.SimConfig(A, S, F, M, pa=pa, p_hardness=p, ibo_db=ibo, snr_db=snr, channel=channel, receiver=receiver,
                        csi_eps=csi, **geometry(A, F))
    return cfg, np.arange(n)


def run_oracle(cfg, trials):
    return sim.run_trials(cfg, SEED, trials, iters=ITERS, incl_clean=True, chunk=4)


@functools.lru_cache(maxsize=None)
def reference(num):
    """The oracle's per-trial counts [trials, 4] of case ``num``; computed once, read-only."""
    cfg, trials = case_config(num)
    ref = run_oracle(cfg, trials)
    ref.setflags(write=False)
    return ref


def band_ratio(cfg):
    """f_k / fc over the data sub-carriers."""
    f = rm.fftfreq_carriers(cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)
    return f[rm.inband_bins(cfg.n_fft, cfg.n_sc)] / f[0]


def antenna_power_spread(cfg):
    """max / min over the antennas of mean_k |H|^2 with the jitter at its centre: the Rayleigh
    attenuation at ``rx_pos``, the LoS / two-path channel at (rx_pos[0], rx_pos[0], rx_pos[2])."""
    bins = rm.inband_bins(cfg.n_fft, cfg.n_sc)
    if cfg.channel == "rayleigh":
        h = rm.fspl_matrix(cfg.tx_pos, cfg.rx_pos, cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)
    else:
        fn = rm.los_channel if cfg.channel == "los" else rm.two_path_channel
        h = fn(cfg.tx_pos, (cfg.rx_pos[0], cfg.rx_pos[0], cfg.rx_pos[2]), cfg.n_fft, cfg.carrier_spacing,
               cfg.center_freq)
    pw = np.mean(np.abs(h[:, bins]) ** 2, axis=1)
    return float(pw.max() / pw.min())


# ---------------------------------------------------------------- mutants of the oracle
# Each is a context manager that patches oracle.refmath / oracle.sim into what a kernel with one
# dropped or misindexed geometry factor would compute, and restores the module on exit.
@contextlib.contextmanager
def _patched(module, name, fn):
    orig = getattr(module, name)
    setattr(module, name, fn(orig))
    try:
        yield
    finally:
        setattr(module, name, orig)


def _rel_freq(n_fft, carrier_spacing, center_freq):
    f = rm.fftfreq_carriers(n_fft, carrier_spacing, center_freq)
    return f / f[0]


def fspl_antennas_reversed():
    """Rayleigh: the free-space attenuation with the antennas in reverse order (``ant_rel[A - 1 - a]``)."""
    return _patched(rm, "fspl_matrix", lambda orig: lambda *a, **k: orig(*a, **k)[::-1].copy())


def fspl_same_for_every_antenna():
    """Rayleigh: every antenna attenuated like the nearest one (``ant_rel`` taken as 1)."""
    def wrap(orig):
        def fn(*a, **k):
            att = orig(*a, **k)
            return np.broadcast_to(att.max(axis=0, keepdims=True), att.shape).copy()
        return fn
    return _patched(rm, "fspl_matrix", wrap)


def fspl_flat_in_frequency():
    """Rayleigh: the attenuation of the centre frequency on every sub-carrier (``f_rel`` taken as 1)."""
    def wrap(orig):
        def fn(*a, **k):
            att = orig(*a, **k)
            return np.broadcast_to(att[:, :1], att.shape).copy()
        return fn
    return _patched(rm, "fspl_matrix", wrap)


def _amplitude_same_for_every_antenna(name):
    def wrap(orig):
        def fn(*a, **k):
            h = orig(*a, **k)
            mag = np.abs(h)
            return h / mag * mag.max(axis=0, keepdims=True)
        return fn
    return _patched(rm, name, wrap)


def los_amplitude_same_for_every_antenna():
    """LoS: the phases kept, the amplitude of the nearest antenna on all of them."""
    return _amplitude_same_for_every_antenna("los_channel")


def _amplitude_flat_in_frequency(name):
    def wrap(orig):
        def fn(tx_pos, rx_pos, n_fft, carrier_spacing, center_freq, *a, **k):
            h = orig(tx_pos, rx_pos, n_fft, carrier_spacing, center_freq, *a, **k)
            return h * _rel_freq(n_fft, carrier_spacing, center_freq)[None, :]  # undoes the 1 / f_k of every path
        return fn
    return _patched(rm, name, wrap)


def los_amplitude_flat_in_frequency():
    """LoS: the phases kept, c / (4 pi d fc) on every sub-carrier."""
    return _amplitude_flat_in_frequency("los_channel")


def two_path_amplitude_flat_in_frequency():
    """Two-path: both paths' phases kept, their amplitudes those of the centre frequency."""
    return _amplitude_flat_in_frequency("two_path_channel")


def y_jittered_around_rx_y():
    """LoS / two-path: the natural reading -- y drawn around ``rx_pos[1]``, not around ``rx_pos[0]``."""
    def wrap(orig):
        def fn(cfg, z_chan, loc_u):
            if cfg.channel not in ("los", "two_path") or not cfg.reroll:
                return orig(cfg, z_chan, loc_u)
            rx = (cfg.rx_pos[0] - cfg.rx_loc_var / 2 + cfg.rx_loc_var * loc_u[0],
                  cfg.rx_pos[1] - cfg.rx_loc_var / 2 + cfg.rx_loc_var * loc_u[1], cfg.rx_pos[2])
            ch = rm.los_channel if cfg.channel == "los" else rm.two_path_channel
            return ch(cfg.tx_pos, rx, cfg.n_fft, cfg.carrier_spacing, cfg.center_freq)[:, rm.inband_bins(cfg.n_fft, cfg.n_sc)]
        return fn
    return _patched(sim, "channel_inband", wrap)


def noise_power_without_frequency_weight(cfg):
    """Every channel: the AGC's mean over the sub-carriers of |sum_a alpha_a H_a P_a|^2, which sets
    the noise power, taken over the channel with its 1 / f_k factored out and the weight
    (fc / f_k)^2 forgotten."""
    w = band_ratio(cfg) ** 2  # (f_k / fc)^2 undoes the weight

    def wrap(orig):
        def fn(*a, **k):
            g = orig(*a, **k)
            g["hk_vk_noise"] = float(np.mean(np.abs(g["hk_vk"]) ** 2 * w))
            g["ak_hk_vk_noise"] = float(np.mean(np.abs(g["ak_hk_vk"]) ** 2 * w))
            return g
        return fn
    return _patched(rm, "agc", wrap)


# name -> (channels it applies to, factory taking the case's SimConfig)
MUTANTS = {
    "fspl_antennas_reversed": (("rayleigh",), lambda cfg: fspl_antennas_reversed()),
    "fspl_same_for_every_antenna": (("rayleigh",), lambda cfg: fspl_same_for_every_antenna()),
    "fspl_flat_in_frequency": (("rayleigh",), lambda cfg: fspl_flat_in_frequency()),
    "los_amplitude_same_for_every_antenna": (("los",), lambda cfg: los_amplitude_same_for_every_antenna()),
    "los_amplitude_flat_in_frequency": (("los",), lambda cfg: los_amplitude_flat_in_frequency()),
    "y_jittered_around_rx_y": (("los", "two_path"), lambda cfg: y_jittered_around_rx_y()),
    "two_path_amplitude_flat_in_frequency": (("two_path",), lambda cfg: two_path_amplitude_flat_in_frequency()),
    "noise_power_without_frequency_weight": (("rayleigh", "los", "two_path"), noise_power_without_frequency_weight),
}


def mutants_for(channel):
    return [name for name, (chans, _) in MUTANTS.items() if channel in chans]


def mutant_counts(num, name, geometry=off_default):
    """The oracle's counts of case ``num`` under mutant ``name``."""
    cfg, trials = case_config(num, geometry)
    with MUTANTS[name][1](cfg):
        return run_oracle(cfg, trials)
