"""Deterministic stand-in for mp_model.Link's coded calls on machines without a GPU: the cells of a
point depend only on (IBO, SNR, trials), so sweep.coded_ber_vs_ebn0 and its CSV writer can be checked
against hand-computed values."""
import types

import numpy as np

import _engine

N_SC, M = 8, 16
N_IDX = 2
N_CODE_BITS, N_CW = 16, 2  # 32 bits per trial: two codewords of 16


def fake_cells(ibo, snr_db, n_trials):
    """Per index k of N_IDX, over the n_trials N_CW frames: ``floor(bits / (4 + 4 k + ibo))`` raw
    errors, a tenth of them (floored) left after the decoder, ``round(snr_db) % 3 + k`` wrong frames
    and k flagged ones."""
    bits = n_trials * N_CW * N_CODE_BITS
    c = np.zeros((N_IDX, _engine.CODED_FIXED))
    for k in range(N_IDX):
        c[k, 0] = np.floor(bits / (4 + 4 * k + ibo))
        c[k, 1] = np.floor(c[k, 0] / 10)
        c[k, 2] = int(round(snr_db)) % 3 + k
        c[k, 3] = k
    return c


class FakeCodedLink:
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

    def coded_points(self, incl_clean_run, reroll_chan, cnc_n_iter_lst, seed_arrs, point_params, n_trials, code,
                     rho_max=None):
        self.calls.append(dict(incl_clean=incl_clean_run, reroll_chan=reroll_chan, iters=list(cnc_n_iter_lst),
                               seeds=list(seed_arrs), ibos=[p["ibo_db"] for p in point_params],
                               snrs=[p["snr_db"] for p in point_params], n_trials=n_trials, code=code,
                               rho_max=rho_max))
        return [_engine.CodedStats(fake_cells(p["ibo_db"], p["snr_db"], n_trials), n_trials * N_CW, N_CODE_BITS)
                for p in point_params]
