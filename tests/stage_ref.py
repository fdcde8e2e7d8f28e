"""Long-double references of the float64 stage kernels (csrc/stages.hip, the object API's
fine seams): OFDM tx / rx, the LLR, MRT, combine, the AWGN values and the CNC loop, each the
formula of oracle/refmath.py restated in np.longdouble on probe_util's ld_fft / ld_pa.
tests/test_stage_ref.py pins every one of them to the float64 oracle at float64 rounding;
tests/test_gpu_stage_kernels.py measures the kernels and the oracle against them."""
import numpy as np

import probe_util as pu
from oracle import philox as px
from oracle import refmath as rm

LD, CLD = pu.LD, pu.CLD
U = 2.0 ** -53  # float64 unit roundoff
PA_CODE = {"none": pu.PA_NONE, "softlim": pu.PA_SOFTLIM, "rapp": pu.PA_RAPP, "toi": pu.PA_TOI}
GRID_PASS = 4096 * 256  # stages.hip grid_for: the elements one pass of the largest grid covers
BIG = GRID_PASS + 257   # one full pass, one full block and a partial block of the second


# ---------------------------------------------------------------- OFDM
def ld_ofdm_tx(symbols, n_fft, n_sub_carr, cp_len):
    """rm.ofdm_tx: bins, ortho IFFT, cyclic prefix."""
    s = np.asarray(symbols, CLD)
    fd = np.zeros(s.shape[:-1] + (n_fft,), CLD)
    fd[..., rm.inband_bins(n_fft, n_sub_carr)] = s
    td = pu.ld_fft(fd, +1) / np.sqrt(LD(n_fft))
    return np.concatenate((td[..., n_fft - cp_len:], td), axis=-1)


def ld_ofdm_rx(td, n_fft, n_sub_carr, cp_len):
    """rm.ofdm_rx: drop the prefix, ortho FFT, in-band bins."""
    fd = pu.ld_fft(np.asarray(td, CLD)[..., cp_len:], -1) / np.sqrt(LD(n_fft))
    return fd[..., rm.inband_bins(n_fft, n_sub_carr)]


# ---------------------------------------------------------------- LLR
def ld_llr(constellation, symbols, noise_var):
    """rm.soft_llr in long double, [n, bits] MSB first.  Long double's exponent range is wider
    than float64's, so a float64 sum that underflows to 0 stays positive here: compare values
    only where the oracle's LLRs are finite."""
    const = np.asarray(constellation, CLD)
    z = np.asarray(symbols, CLD).reshape(-1)
    nv = np.broadcast_to(np.asarray(noise_var, LD), z.shape)
    d = z[:, None] - const[None, :]
    metric = np.exp(-(d.real * d.real + d.imag * d.imag) / nv[:, None])
    n_bits = rm.bits_per_symbol(len(const))
    labels = np.arange(len(const))
    out = np.empty((z.size, n_bits), LD)
    for b in range(n_bits):
        ones = ((labels >> b) & 1).astype(bool)
        out[:, n_bits - 1 - b] = np.log(metric[:, ones].sum(axis=1) / metric[:, ~ones].sum(axis=1))
    return out


def llr_exponents(constellation, symbols, noise_var):
    """-|z - C|^2 / nv per (point, label) in float64: what the +-inf pattern depends on."""
    const = np.asarray(constellation)
    z = np.asarray(symbols).reshape(-1)
    nv = np.broadcast_to(np.asarray(noise_var, np.float64), z.shape)
    return -np.abs(z[:, None] - const[None, :]) ** 2 / nv[:, None]


# ---------------------------------------------------------------- MRT / combine
def ld_mrt(h):
    """rm.mrt_precoding for [A, K]."""
    h = np.asarray(h, CLD)
    s = np.sum(h.real * h.real + h.imag * h.imag, axis=0, keepdims=True)
    return np.conjugate(h) / np.sqrt(s)


def ld_combine(h, y):
    """(sum_a h_a y_a, sum_a |h_a| |y_a|) per column of [A, K]: the value and the scale its
    rounding error is measured by (a sum that cancels has a small value and a large scale)."""
    h, y = np.asarray(h, CLD), np.asarray(y, CLD)
    return np.sum(h * y, axis=0), np.sum(np.abs(h) * np.abs(y), axis=0)


# ---------------------------------------------------------------- AWGN
def awgn_words(seed, counter, idx):
    """Philox words (w0, w1) of element idx: counter (i_lo, ctr_lo, 6, ctr_hi ^ i_hi), key seed."""
    i = np.asarray(idx, np.uint64)
    counter = int(counter)
    w = px.philox4x32_10(i & px.MASK, counter & 0xFFFFFFFF, 6,
                         np.uint64((counter >> 32) & 0xFFFFFFFF) ^ (i >> px.S32), int(seed))
    return w[0], w[1]


def ld_awgn_noise(seed, counter, idx, noise_std):
    """The noise mimo_awgn adds to element idx: BoxMuller(w0, w1) std / sqrt(2), long double."""
    w0, w1 = awgn_words(seed, counter, idx)
    u1 = (w0.astype(LD) + LD(0.5)) * LD(2.0 ** -32)
    u2 = w1.astype(LD) * LD(2.0 ** -32)
    rho = np.sqrt(-np.log(u1))
    ang = 2 * pu.LD_PI * u2
    return (rho * np.cos(ang) + CLD(1j) * (rho * np.sin(ang))) * (LD(noise_std) / np.sqrt(LD(2)))


def np_awgn_noise(seed, counter, idx, noise_std):
    """The same in float64 by the oracle's box_muller: the yardstick."""
    w0, w1 = awgn_words(seed, counter, idx)
    return px.box_muller(w0, w1) * (noise_std / np.sqrt(2.0))


# ---------------------------------------------------------------- CNC
def slicer_margin(v, constel_size):
    """Smallest distance of the points v (either axis) from a decision boundary of the square
    constellation: the even integers strictly inside (-L, L)."""
    L = int(round(np.sqrt(constel_size)))
    bounds = np.arange(-L + 2, L - 1, 2).astype(np.float64)
    v = np.asarray(v, np.complex128).reshape(-1)
    ax = np.concatenate((v.real, v.imag))
    return float(np.min(np.abs(ax[:, None] - bounds[None, :])))


def ld_cnc_receive(n_iters_lst, rx_nsc, constellation, n_fft, pa_kind, sat, p_hardness, coeff, alpha):
    """rm.cnc_receive in long double (ld_fft, ld_pa, the brute-force slicer on the long-double
    slicer input).  -> ({iteration: labels}, {iteration: slicer input rx - d}) for EVERY
    iteration up to the last listed one."""
    rx = np.asarray(rx_nsc, CLD)
    n_sc = rx.shape[-1]
    bins = rm.inband_bins(n_fft, n_sc)
    const = np.asarray(constellation)
    labs, vs = {}, {}
    d = None
    last = int(np.max(n_iters_lst))
    for it in range(last + 1):
        v = rx if it == 0 else rx - d
        lab = rm.detect_labels(const, v)
        labs[it], vs[it] = lab, v
        if it == last:
            break
        s_hat = const[lab].astype(CLD)
        up = np.zeros(n_fft, CLD)
        up[bins] = s_hat
        td = pu.ld_fft(up, +1) / np.sqrt(LD(n_fft))
        td = pu.ld_pa(PA_CODE[pa_kind], td, sat, p_hardness, coeff)
        est = (pu.ld_fft(td, -1) / np.sqrt(LD(n_fft)))[bins] / LD(alpha)
        d = est - s_hat
    return labs, vs


# ---------------------------------------------------------------- metrics
def rel_err(got, ref):
    """|got - ref| / |ref| per element, formed in long double; where ref = 0 the entry is 0 if
    got equals it bit for bit (either zero sign) and inf otherwise."""
    got, ref = np.asarray(got, CLD), np.asarray(ref, CLD)
    a = np.abs(ref)
    out = np.where(a > 0, np.abs(got - ref) / np.where(a > 0, a, LD(1)), np.where(got == ref, LD(0), LD(np.inf)))
    return np.asarray(out, np.float64)
