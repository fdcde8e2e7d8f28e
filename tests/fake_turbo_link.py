"""Deterministic stand-in for mp_model.Link's turbo calls on machines without a GPU: the cells of a
point depend only on (IBO, SNR, trials, passes), so sweep.turbo_ber_vs_ebn0 and its CSV writer can be
checked against hand-computed values."""
import types

import numpy as np

import _engine

N_SC, M = 8, 16
N_CODE_BITS, N_CW = 16, 2  # 32 bits per trial: two codewords of 16


def fake_cells(ibo, snr_db, n_trials, n_passes):
    """Per pass q, over the n_trials N_CW frames: ``floor(bits / (4 + 4 q + ibo))`` raw errors, a tenth
    of them (floored) left after the decoder, ``round(snr_db) % 3 + q`` wrong frames and q flagged ones."""
    bits = n_trials * N_CW * N_CODE_BITS
    c = np.zeros((n_passes, _engine.CODED_FIXED))
    for q in range(n_passes):
        c[q, 0] = np.floor(bits / (4 + 4 * q + ibo))
        c[q, 1] = np.floor(c[q, 0] / 10)
        c[q, 2] = int(round(snr_db)) % 3 + q
        c[q, 3] = q
    return c


class FakeTurboLink:
    my_mod = types.SimpleNamespace(n_sub_carr=N_SC, constel_size=M)

    def __init__(self):
        self.ibo = self.snr = None
        self.calls = []

    def update_distortion(self, ibo_val_db):
        self.ibo = ibo_val_db

    def set_snr(self, snr_db):
        self.snr = snr_db

    def point_params(self):
        return dict(ibo_db=self.ibo, snr_db=self.snr)

    def turbo_points(self, reroll_chan, seed_arrs, point_params, n_trials, code, n_passes, rho_max=None):
        self.calls.append(dict(reroll_chan=reroll_chan, seeds=list(seed_arrs), ibos=[p["ibo_db"] for p in point_params],
                               snrs=[p["snr_db"] for p in point_params], n_trials=n_trials, code=code,
                               n_passes=n_passes, rho_max=rho_max))
        return [_engine.TurboStats(fake_cells(p["ibo_db"], p["snr_db"], n_trials, n_passes), n_trials * N_CW, N_CODE_BITS)
                for p in point_params]
