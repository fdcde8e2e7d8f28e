"""Deterministic stand-in for mp_model.Link's soft calls on machines without a GPU: the histogram
of a point depends only on (IBO, SNR, trials), so sweep.gmi_vs_ebn0 and its CSV writer can be
checked against hand-computed values."""
import types

import numpy as np

import _engine

N_SC, M = 8, 16
N_IDX = 2


def fake_hist(ibo, snr_db, n_trials):
    """Per index k of N_IDX: of the n = n_trials N_SC log2 M reliabilities, 1 / (4 + 4 k + ibo) fall in
    bin 127 (errors of half a bin width) and the rest in bin 128 + round(snr_db) (right by that many
    and a half)."""
    n = n_trials * N_SC * 4
    h = np.zeros((N_IDX, _engine.SOFT_BINS))
    for k in range(N_IDX):
        bad = np.floor(n / (4 + 4 * k + ibo))
        h[k, 127] = bad
        h[k, 128 + int(round(snr_db))] = n - bad
    return h


class FakeSoftLink:
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

    def soft_points(self, incl_clean_run, reroll_chan, cnc_n_iter_lst, seed_arrs, point_params, n_trials,
                    rho_max=None):
        self.calls.append(dict(incl_clean=incl_clean_run, reroll_chan=reroll_chan, iters=list(cnc_n_iter_lst),
                               seeds=list(seed_arrs), ibos=[p["ibo_db"] for p in point_params],
                               snrs=[p["snr_db"] for p in point_params], n_trials=n_trials, rho_max=rho_max))
        return [_engine.SoftStats(fake_hist(p["ibo_db"], p["snr_db"], n_trials), 128.0 if rho_max is None else rho_max,
                                  M, n_trials) for p in point_params]
