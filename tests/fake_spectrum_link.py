"""Deterministic stand-in for mp_model.Link's spectrum calls on machines without a GPU: the row
of a point depends only on (IBO, seed, trials), so sweep.spectrum_vs_ibo and the psd_vs_ibo CSV
writers can be checked against hand-computed values."""
import numpy as np

import _engine

N_FFT, N_SC = 16, 8


class FakeModem:
    n_sub_carr, n_fft, constel_size = N_SC, N_FFT, 16


def fake_row(ibo, n_trials):
    """In-band bins carry n_trials each, out-of-band bins (DC included) n_trials 10^(-(20 + ibo)/10);
    Ex = 2 n_trials S, C = (1 - 0.1 / (1 + ibo)) Ex / 2 (1 + 0.5j)."""
    row = np.full(N_FFT + _engine.SPEC_FIXED, n_trials * 10.0 ** (-(20.0 + ibo) / 10.0))
    row[_engine.inband_bins(N_FFT, N_SC)] = float(n_trials)
    ex = 2.0 * n_trials * N_SC
    c = (1.0 - 0.1 / (1.0 + ibo)) * ex / 2.0 * complex(1.0, 0.5)
    row[N_FFT:] = [ex, c.real, c.imag]
    return row


class FakeSpectrumLink:
    my_mod = FakeModem()

    def __init__(self):
        self.ibo = None
        self.calls = []

    def update_distortion(self, ibo_val_db):
        self.ibo = ibo_val_db

    def point_params(self):
        return dict(ibo_db=self.ibo, snr_db=None)

    def spectrum_points(self, reroll_chan, seed_arrs, point_params, n_trials):
        self.calls.append(dict(reroll_chan=reroll_chan, seeds=list(seed_arrs), ibos=[p["ibo_db"] for p in point_params],
                               n_trials=n_trials))
        return [_engine.SpectrumStats(fake_row(p["ibo_db"], n_trials), N_SC, n_trials) for p in point_params]
