"""Deterministic stand-in for mp_model.Link's envelope calls on machines without a GPU: the row of a
point depends only on (IBO, trials), so sweep.envelope_vs_ibo and the ccdf_vs_ibo CSV writer can be
checked against hand-computed values."""
import numpy as np

import _engine

N_ANT, N_FFT = 2, 16
IN_BINS = (90, 96, 100, 104)  # a quarter of the input samples in each


def clip_bin(ibo):
    """The bin the fake limiter folds the input's tail into: 96 at IBO 0, 8 bins per 3 dB."""
    return 96 + int(round(ibo * 8 / 3))


def fake_row(ibo, n_trials):
    """Input: n / 4 samples in each of IN_BINS (n = n_trials N_ANT N_FFT).  Output: the same, with
    everything above clip_bin(ibo) moved into it.  Pin = 2 n, Pout = (1 - 0.2 / (1 + ibo)) Pin,
    C = (1 - 0.1 / (1 + ibo)) Pin (1 + 0.5j)."""
    n = n_trials * N_ANT * N_FFT
    row = np.zeros(_engine.ENV_WIDTH)
    for b in IN_BINS:
        row[b] += n / 4
        row[_engine.ENV_BINS + min(b, clip_bin(ibo))] += n / 4
    pin = 2.0 * n
    c = (1.0 - 0.1 / (1.0 + ibo)) * pin * complex(1.0, 0.5)
    row[2 * _engine.ENV_BINS:] = [pin, (1.0 - 0.2 / (1.0 + ibo)) * pin, c.real, c.imag]
    return row


class FakeEnvelopeLink:
    def __init__(self):
        self.ibo = None
        self.calls = []

    def update_distortion(self, ibo_val_db):
        self.ibo = ibo_val_db

    def point_params(self):
        return dict(ibo_db=self.ibo, snr_db=None)

    def envelope_points(self, reroll_chan, seed_arrs, point_params, n_trials, ref_pow=None):
        self.calls.append(dict(reroll_chan=reroll_chan, seeds=list(seed_arrs), ibos=[p["ibo_db"] for p in point_params],
                               n_trials=n_trials, ref_pow=ref_pow))
        return [_engine.EnvelopeStats(fake_row(p["ibo_db"], n_trials), N_ANT, N_FFT, n_trials,
                                      2.0 if ref_pow is None else ref_pow) for p in point_params]
