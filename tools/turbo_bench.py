"""Cost of the turbo mode: HIP-event time of the turbo-instance trial kernel against the plain trial
kernel on the same engine, and of the pass loop (step kernels and decoders), at BASELINE config 2
(A 64, S 1024, F 2048) and at the paper geometry (A 64, S 2048, F 4096), float64, 64-QAM, per 1,024
trials, with ``n_passes`` 1 and 4.  The code is utilities.qc_ldpc_code(512, 3, 6) with 10 decoder
iterations: N 3,072, 2 codewords per trial and pass at config 2 and 4 at the paper geometry.  The
counts record CNC iteration 0 alone, so the trial kernels run no CNC iteration of their own.

Per round one child process: per workload a warm-up call of each kind, then --repeats rounds of
calls, plain, turbo at 1 pass and turbo at 4 passes alternating.  Prints one JSON line (--out writes
it to a file as well).

--split DIR: instead, one child under ``rocprofv3 --kernel-trace --stats`` (a run of its own: the
tracer's overhead is in no event time above), whose per-kernel totals split the pass loop into the
step kernels (first pass, later passes) and the two decoder kernels; the statistics are copied to
DIR and summarised in the JSON line.  Every kernel's total is divided by the trials it covered, which
follow from the calls the child makes and not from its launches (a call may run in several launches):
the trial and step kernels carry their FFT size in their names and are given per 1,024 trials of
their workload, the decoder kernels serve both workloads and are given per 1,024 decodes.

Every child runs under its own time limit (--limit seconds); if one is killed or fails, nothing
else is started.

    python tools/turbo_bench.py [--trials 8192] [--repeats 5] [--rounds 3] [--out FILE] [--split DIR]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "m-mimo-ofdm-with-nonlinear-pa-sim_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = ("2", "paper")
ITERS = [0]
PASSES = (1, 4)
TAG = "TURBO_BENCH_CHILD "


def child(a):
    import _engine
    import bench
    from utilities import qc_ldpc_code
    code = qc_ldpc_code(512, 3, 6, n_dec_iters=10)
    out = {}
    for w in WORKLOADS:
        eng = bench.make_engine(0, w, "f64")
        pt = eng._point
        rho_max = 32.0 * pt.avg_symbol_power / (4.0 * 10 ** (pt.snr_db / 10))  # Link.turbo's default range
        n_cw = eng.coded_codewords(code)
        err, _, _ = eng.run(7, 0, a.trials, ITERS)
        cells = {}
        for n in PASSES:
            err_t, _, cells[n], _, _ = eng.turbo(7, 0, a.trials, ITERS, code, rho_max, n)
            assert list(err) == list(err_t)  # the same trials, the same counts
        ms = {"plain_ms": []}
        for n in PASSES:
            ms["turbo%d_ms" % n], ms["loop%d_ms" % n] = [], []
        for _ in range(a.repeats):
            eng.run(7, 0, a.trials, ITERS)
            ms["plain_ms"].append(eng.kernel_ms)
            for n in PASSES:
                eng.turbo(7, 0, a.trials, ITERS, code, rho_max, n)
                ms["turbo%d_ms" % n].append(eng.kernel_ms)
                ms["loop%d_ms" % n].append(eng.decode_kernel_ms)
        st = _engine.TurboStats(cells[PASSES[-1]], a.trials * n_cw, code.n_bits)
        out[w] = dict(describe=eng.describe(), rho_max=rho_max, n_cw=n_cw, raw_ber=st.raw_ber().tolist(),
                      ber=st.ber().tolist(), fer=st.fer().tolist(),
                      pass0_equals_errors=bool(cells[1][0, 0] == err[0]), **ms)  # every position is decoded here
        eng.close()
    print(TAG + json.dumps(out))


def run_child(cmd, limit):
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"a GPU step ran into its limit of {limit:.0f} s")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"a GPU step failed (exit status {r.returncode})")
    return json.loads(line[0][len(TAG):])


def covered(a, name, c):
    """(units a kernel's total covers in one traced child, the unit, the workload or None): per
    workload the child makes 1 + repeats calls of each kind -- plain, turbo at every number of PASSES."""
    calls = 1 + a.repeats
    m = re.search(r"trial_kernel<(\d+), double, (\d+),", name)
    s = re.search(r"turbo_step<(\d+), \d+, (?:true|false), (true|false)>", name)
    fft = int(m.group(2)) if m else int(s.group(1)) if s else None
    w = next((k for k in WORKLOADS if fft is not None and "F=%d " % fft in c[k]["describe"]), None)
    if m and w:  # the plain instance: the plain calls; the turbo instance: one call per entry of PASSES
        return calls * a.trials * (len(PASSES) if int(m.group(1)) == 7 else 1), "trials", w
    if s and w:  # the pass-0 step once per turbo call, the later step once per pass after it
        n = len(PASSES) if s.group(2) == "true" else sum(p - 1 for p in PASSES)
        return calls * a.trials * n, "trials", w
    if "k_ldpc_decode<" in name:
        # (launch_ldpc: the instance with decisions wherever the row stride is not the coded mode's,
        # that is in every pass of a call of more than one pass)
        passes = sum(p for p in PASSES if (p > 1) == ("k_ldpc_decode<true" in name))
        return calls * a.trials * passes * sum(c[k]["n_cw"] for k in WORKLOADS), "decodes", None
    return None, None, None


def split(a, cmd):
    """The kernels of one traced child by name: calls, total time, and time per 1,024 units covered."""
    with tempfile.TemporaryDirectory() as tmp:
        c = run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--"] + cmd,
                  a.limit)
        found = glob.glob(os.path.join(tmp, "**", "run_kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("the tracer left no run_kernel_stats.csv")
        os.makedirs(a.split, exist_ok=True)
        shutil.copy(found[0], os.path.join(a.split, "kernel_stats.csv"))
        with open(found[0]) as f:
            rows = list(csv.DictReader(f))
    groups = {"trial_kernel": "trial kernels (plain and turbo instances)", "turbo_step": "step kernels",
              "k_ldpc_decode<true": "decoder with decisions", "k_ldpc_decode<false": "decoder"}
    out = {v: dict(calls=0, total_ms=0.0) for v in groups.values()}
    for r in rows:
        for key, name in groups.items():
            if key in r["Name"]:
                out[name]["calls"] += int(r["Calls"])
                out[name]["total_ms"] += int(r["TotalDurationNs"]) / 1e6
                break
    kernels = []
    for r in rows:
        if "mimo" not in r["Name"]:
            continue
        k = dict(name=r["Name"], calls=int(r["Calls"]), total_ms=int(r["TotalDurationNs"]) / 1e6,
                 average_us=float(r["AverageNs"]) / 1e3)
        n, unit, w = covered(a, r["Name"], c)
        if n:
            k.update({unit: n, "ms_per_1024_" + unit: k["total_ms"] * 1024.0 / n}, **({"workload": w} if w else {}))
        kernels.append(k)
    return dict(kernels=kernels, groups=out, n_cw={w: c[w]["n_cw"] for w in WORKLOADS})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trials", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one GPU child process [s]")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--split", type=str, default=None, help="directory for the kernel-trace statistics")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--trials", str(a.trials), "--repeats", str(a.repeats)]
    if a.split:
        s = json.dumps(dict(trials=a.trials, repeats=a.repeats, passes=PASSES, **split(a, cmd)))
    else:
        series = ["plain_ms"] + ["%s%d_ms" % (k, n) for n in PASSES for k in ("turbo", "loop")]
        res = {w: {k: [] for k in series} for w in WORKLOADS}
        for _ in range(a.rounds):
            c = run_child(cmd, a.limit)
            for w in WORKLOADS:
                for k in ("describe", "rho_max", "n_cw", "raw_ber", "ber", "fer", "pass0_equals_errors"):
                    res[w][k] = c[w][k]
                for k in series:
                    res[w][k] += c[w][k]
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        per = 1024.0 / a.trials
        for w in WORKLOADS:
            d = res[w]
            for k in series:
                d[k[:-3] + "_ms_per_1024"] = med(d[k]) * per
                d[k[:-3] + "_spread"] = (max(d[k]) - min(d[k])) / med(d[k])
            for n in PASSES:
                d["turbo%d_over_plain" % n] = med(d["turbo%d_ms" % n]) / med(d["plain_ms"])
            d["later_pass_ms_per_1024"] = (med(d["loop4_ms"]) - med(d["loop1_ms"])) * per / 3.0
        s = json.dumps(dict(trials=a.trials, repeats=a.repeats, rounds=a.rounds, workloads=res))
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
