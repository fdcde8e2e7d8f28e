"""The float64 wave-split instances (F 1024 on T 128, F 2048 on T 256; csrc/wave_fft.h) as a case
table, their cached references for all seven run modes, and which instances hold their transform
addresses across the antenna loop (csrc/trial_kernel.h xaddr_inst_ok).  No GPU.

These two sizes are the hot path and the sizes whose instances differ most from one another: per
(F, mode, aligned, channel) an instance holds its addresses or re-derives them, and each is its own
compilation.  One family per (F, slot class, channel, CSI), 2 x 2 x 4 x 2 = 32; every family runs
in all seven modes, which reaches each of the 224 kernels once.

  aligned band   S = F / 2: 4 slots
  generic band   S = 500 at F 1024, S = 1000 at F 2048: 8 slots (engine.hip select_instance), a band
                 that is no multiple of a wave, of T, or of 4 T
  A = 3          more than one antenna, so held addresses are reused, and no multiple of the wave count
  16-QAM, soft limiter at IBO 3 dB, Es/N0 16 dB, trials 0-3, CNC / MCNC iterations 0, 1, 2 and the
  clean column: the geometry of tests/test_gpu_wave_balance.py SHAPES["F1024"]
  table          one random table scaled as tests/test_gpu_bank.py tables(), reroll off

``tests/test_wave_split_cases.py`` pins the conditions that make the table worth running, on the
references alone; ``tests/test_gpu_wave_split_instances.py`` runs it on the device.
"""
import dataclasses
import functools
import os
import re

import numpy as np

import _engine
import beam_ref
import envelope_ref
import ldpc_ref
import measure_ref
import soft_ref
import spectrum_ref
from oracle import sim
from test_gpu_bank import tables
from test_gpu_beam import probes_n
from test_gpu_coded import CASES as CODED_CASES
from test_gpu_coded import N_DEC, TABLES
from test_gpu_soft import CASES as SOFT_CASES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "m-mimo-ofdm-with-nonlinear-pa-sim_amd", "csrc")

SIZES = {1024: 128, 2048: 256}                       # F -> T of the float64 instance
GENERIC_S = {1024: 500, 2048: 1000}
CHANNELS = ("rayleigh", "los", "two_path", "table")
CSI_EPS = (None, 0.2)
N_ANT, CONSTEL = 3, 16
IBO_DB, SNR_DB = 3.0, 16.0
TRIALS = 4
ITERS = (0, 1, 2)        # counters: clean + these
N_PROBES = 5
MODES = ("plain", "measure", "spectrum", "beam", "envelope", "soft", "coded")  # index: MIMO_MODE_*
ROW_MODES = MODES[1:]

# the code and rho_max of tests/test_gpu_coded.py's smallest case
_SOFT_NAME, CODE_KEY, _, _ = CODED_CASES["f128_qpsk-z16"]
RHO_MAX = SOFT_CASES[_SOFT_NAME][3]

SEED = 7
# (F, aligned, channel, csi) -> the next integer, where SEED misses a condition of
# tests/test_wave_split_cases.py for that family
SEEDS = {}


@dataclasses.dataclass(frozen=True)
class Family:
    n_fft: int
    aligned: bool
    channel: str
    csi_eps: float | None

    @property
    def key(self):
        return (self.n_fft, self.aligned, self.channel, self.csi_eps is not None)

    @property
    def n_sc(self):
        return self.n_fft // 2 if self.aligned else GENERIC_S[self.n_fft]

    @property
    def slots(self):
        """engine.hip select_instance: S / T of an aligned band, else the F / T points of a thread."""
        t = SIZES[self.n_fft]
        return self.n_sc // t if self.aligned else self.n_fft // t

    @property
    def ch(self):
        return _engine.CH_KINDS[self.channel]

    @property
    def seed(self):
        return SEEDS.get(self.key, SEED)

    @property
    def describe(self):
        """The text ``Engine.describe()`` must return for this family."""
        return (f"F={self.n_fft} T={SIZES[self.n_fft]} slots={self.slots} {'aligned' if self.aligned else 'generic'} "
                f"ch={self.ch} csi={int(self.csi_eps is not None)} f64")

    @property
    def id(self):
        return (f"F{self.n_fft}-{'aligned' if self.aligned else 'generic'}-{self.channel}"
                + ("" if self.csi_eps is None else "-csi"))

    # A family that mimo_engine_create refuses carries the expected error text here, and the device
    # test asserts the refusal.  validate_config (engine.hip) accepts all 32: table + CSI runs with a
    # single table.
    refused = None

    def config(self, receiver="cnc"):
        kw = {}
        if self.channel == "table":
            kw = dict(table_h=tables(1, N_ANT, self.n_fft)[0], reroll=False)
        return sim.SimConfig(N_ANT, self.n_sc, self.n_fft, CONSTEL, pa="softlim", ibo_db=IBO_DB, snr_db=SNR_DB,
                             channel=self.channel, receiver=receiver, csi_eps=self.csi_eps, **kw)


FAMILIES = [Family(f, al, ch, csi) for f in SIZES for al in (True, False) for ch in CHANNELS for csi in CSI_EPS]
BY_ID = {fam.id: fam for fam in FAMILIES}
# the generic families whose six row modes also run under MCNC
MCNC_ROW_FAMILIES = ("F1024-generic-los", "F2048-generic-table")


def _trials():
    return np.arange(TRIALS)


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_code():
    z, table = TABLES[CODE_KEY]
    return ldpc_ref.Code(z, np.array(table()), N_DEC)


@functools.lru_cache(maxsize=None)
def ref_pow(fam):
    """The envelope mode's reference power: the nominal mean sample power."""
    return envelope_ref.nominal_power(fam.config())


def reference(fam, mode="plain", receiver="cnc"):
    """The reference of a family in a mode, computed once, its arrays read-only:
      plain     counts [trials, 4], the oracle's (oracle/sim.py run_trials)
      measure   (counts, rows, Ez)                          measure_ref.reference_rows
      spectrum  (counts, rows)                              spectrum_ref.reference_rows
      beam      (counts, rows, bounds)                      beam_ref.reference_rows, probes_n(5)
      envelope  (counts, rows, near-edge samples)           envelope_ref.reference at ref_pow(fam)
      soft      (counts, rows, near-edge, zeros)            soft_ref.reference at RHO_MAX
      coded     (counts, chan, rows, decoded-position errors, near-edge, zeros)   ldpc_ref.reference
    """
    return _reference(fam, mode, receiver)


@functools.lru_cache(maxsize=None)
def _reference(fam, mode, receiver):
    cfg, seed, tr = fam.config(receiver), fam.seed, _trials()
    if mode == "plain":
        ref = sim.run_trials(cfg, seed, tr, iters=ITERS, incl_clean=True)
        ref.setflags(write=False)
        return ref
    if mode == "measure":
        return _frozen(measure_ref.reference_rows(cfg, seed, tr, ITERS, True))
    if mode == "spectrum":
        return _frozen(spectrum_ref.reference_rows(cfg, seed, tr, ITERS, True))
    if mode == "beam":
        return _frozen(beam_ref.reference_rows(cfg, seed, tr, ITERS, probes_n(N_PROBES), True))
    if mode == "envelope":
        return _frozen(envelope_ref.reference(cfg, seed, tr, ITERS, ref_pow(fam), True))
    if mode == "soft":
        return _frozen(soft_ref.reference(cfg, seed, tr, ITERS, RHO_MAX, True))
    if mode == "coded":
        return _frozen(ldpc_ref.reference(cfg, ref_code(), seed, tr, ITERS, RHO_MAX, True))
    raise ValueError(mode)


# ---------------------------------------------------------------- which instances hold their addresses
@functools.lru_cache(maxsize=None)
def left_out_masks():
    """{F: the seven per-mode masks} of xaddr_inst_ok (csrc/trial_kernel.h), read from the source
    text: bit (aligned ? 0 : 4) + channel kind - 1 set = that instance keeps re-deriving."""
    with open(os.path.join(CSRC, "trial_kernel.h")) as f:
        src = f.read()
    out = {}
    for size in SIZES:
        m = re.search(r"constexpr unsigned out%d\[7\] = \{([^}]*)\};" % size, src)
        out[size] = tuple(int(v, 0) for v in m.group(1).split(","))
        assert len(out[size]) == len(MODES)
    return out


def holds_addresses(n_fft, mode, aligned, ch, csi=False):
    """Whether the float64 instance (F, mode index or name, slot class, MIMO_CH_* kind) holds its
    transforms' addresses across the antenna loop; a CSI instance never does (trial_kernel.h XADDR)."""
    mode = MODES.index(mode) if isinstance(mode, str) else int(mode)
    if csi or n_fft not in SIZES or not 0 <= mode < len(MODES) or not 1 <= ch <= 4:
        return False
    bit = 1 << ((0 if aligned else 4) + ch - 1)
    return not left_out_masks()[n_fft][mode] & bit


def held(fam, mode):
    return holds_addresses(fam.n_fft, mode, fam.aligned, fam.ch, fam.csi_eps is not None)
