"""Cost of the beam mode at BASELINE config 2's geometry (A 64, S 1024, F 2048, float64): 181 probes on
the half circle through the user, 1024 trials per call; a warm-up call, then --repeats calls.

Reports the HIP-event time of the beam-instance trial kernel and of the beamforming kernel
(csrc/beam.hip) separately, the plain trial kernel's for comparison, the beamforming kernel's achieved
float64 rate from 8 N_q A (F + S) flops per trial against the 78.6 TF vector peak, and the bytes it
reads against the HBM bandwidth, and prints one JSON line (--out writes it to a file as well).

The GPU work runs in a child process under its own time limit (--limit seconds); if the child is
killed or fails, nothing else is started.

    python tools/beam_bench.py [--trials 1024] [--probes 181] [--repeats 5] [--out FILE]
"""
import argparse
import json
import math
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "m-mimo-ofdm-with-nonlinear-pa-sim_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F64_TFLOPS = 78.6   # MI355X vector float64
HBM_TBPS = 6.3           # achievable HBM3E bandwidth (8.0 spec)
BEAM_QB, BEAM_TT = 8, 4  # csrc/beam.hip: probes per block (4 waves x kBeamQT), trials per block


def child(a):
    import numpy as np

    import bench
    from utilities import circle_probes
    w = bench.WORKLOADS["2"]
    eng = bench.make_engine(0, "2", "f64")
    probes = circle_probes(np.linspace(0.0, 180.0, a.probes), math.hypot(212.0, 212.0), 1.5)
    eng.beam(7, 0, a.trials, [0], probes)  # warm-up: module load, buffers
    trial_ms, beam_ms = [], []
    for _ in range(a.repeats):
        eng.beam(7, 0, a.trials, [0], probes)
        trial_ms.append(eng.kernel_ms)
        beam_ms.append(eng.beam_kernel_ms)
    eng.run(7, 0, a.trials, [0])
    plain_ms = []
    for _ in range(a.repeats):
        eng.run(7, 0, a.trials, [0])
        plain_ms.append(eng.kernel_ms)
    print("BEAM_BENCH_CHILD " + json.dumps(dict(A=w["A"], S=w["S"], F=w["F"], describe=eng.describe(),
                                                trial_ms=trial_ms, beam_ms=beam_ms, plain_ms=plain_ms)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trials", type=int, default=1024)
    ap.add_argument("--probes", type=int, default=181)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="time limit of the GPU child process [s]")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--trials", str(a.trials), "--probes", str(a.probes),
           "--repeats", str(a.repeats)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the GPU step ran into its limit of {a.limit:.0f} s")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BEAM_BENCH_CHILD ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"the GPU step failed (exit status {r.returncode})")
    c = json.loads(line[0][len("BEAM_BENCH_CHILD "):])
    A, S, F, nq, nt = c["A"], c["S"], c["F"], a.probes, a.trials
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    beam_ms, trial_ms, plain_ms = med(c["beam_ms"]), med(c["trial_ms"]), med(c["plain_ms"])
    flops = 8.0 * nq * A * (F + S) * nt
    unique = 16.0 * A * (F + S) * nt                    # every Y cell and every in-band X cell once
    requested = unique * math.ceil(nq / BEAM_QB)        # ... once per block of probes (4 waves share the L1)
    t_flops, t_hbm = flops / (PEAK_F64_TFLOPS * 1e12) * 1e3, unique / (HBM_TBPS * 1e12) * 1e3
    t_hbm_nocache = requested / (HBM_TBPS * 1e12) * 1e3
    out = dict(workload=f"A {A} S {S} F {F} float64, {nq} probes, {nt} trials", instance=c["describe"],
               repeats=a.repeats, trial_kernel_beam_ms=trial_ms, trial_kernel_plain_ms=plain_ms,
               beamforming_kernel_ms=beam_ms, all_beam_ms=c["beam_ms"], all_trial_ms=c["trial_ms"],
               all_plain_ms=c["plain_ms"], beamforming_tflops=flops / (beam_ms * 1e-3) / 1e12,
               share_of_f64_peak=flops / (beam_ms * 1e-3) / 1e12 / PEAK_F64_TFLOPS,
               bytes_unique=unique, bytes_requested_by_blocks=requested,
               unique_tbps=unique / (beam_ms * 1e-3) / 1e12, requested_tbps=requested / (beam_ms * 1e-3) / 1e12,
               ms_at_f64_peak=t_flops, ms_at_hbm_unique=t_hbm, ms_at_hbm_if_nothing_cached=t_hbm_nocache,
               nearer_bound="float64 rate" if t_flops >= t_hbm else "HBM bandwidth")
    s = json.dumps(out)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
