"""Deterministic stand-in for mp_model.Link's beampattern calls on machines without a GPU: the rows
of a point depend only on (IBO, trials, probe index), so sweep.beam_vs_angle and its CSV writer can
be checked against hand-computed values."""
import numpy as np

import _engine


class FakeRx:
    cord_x, cord_y, cord_z = 3.0, 4.0, 1.5  # on the circle of radius 5


def fake_rows(ibo, n_trials, n_probes):
    """Probe i: Px = 4 n, C = (2 + i) n, so signal = (2 + i)^2 n / 4; distortion = n / (2 (1 + ibo));
    Py_oob = (1 + i) n / 100."""
    i = np.arange(n_probes, dtype=np.float64)
    n = float(n_trials)
    sig = (2.0 + i) ** 2 * n / 4.0
    return np.stack([sig + n / (2.0 * (1.0 + ibo)), (1.0 + i) * n / 100.0, np.full(n_probes, 4.0 * n), (2.0 + i) * n,
                     np.zeros(n_probes)], axis=1)


class FakeBeamLink:
    my_standard_rx = FakeRx()

    def __init__(self):
        self.ibo = None
        self.calls = []

    def update_distortion(self, ibo_val_db):
        self.ibo = ibo_val_db

    def point_params(self):
        return dict(ibo_db=self.ibo, snr_db=None)

    def beampattern_points(self, reroll_chan, seed_arrs, point_params, n_trials, probes):
        probes = np.asarray(probes)
        self.calls.append(dict(reroll_chan=reroll_chan, seeds=list(seed_arrs), ibos=[p["ibo_db"] for p in point_params],
                               n_trials=n_trials, probes=probes.copy()))
        return [_engine.BeamStats(fake_rows(p["ibo_db"], n_trials, len(probes)), n_trials) for p in point_params]
