"""Cost of the soft mode: HIP-event time of the soft-instance trial kernel against the plain trial
kernel on the same engine, at BASELINE config 2 (A 64, S 1024, F 2048) and at the paper geometry
(A 64, S 2048, F 4096), float64, 64-QAM, CNC iterations 0-4 all recorded, per 1,024 trials.

Per library and round one child process: per workload a warm-up call of each mode, then --repeats
pairs of calls, plain and soft alternating.  With several --libs (A/B builds of the soft instances,
e.g. -DMIMO_DIAG_SOFT_NOHIST) the libraries alternate round by round, so that they share the
machine's drift.  Prints one JSON line (--out writes it to a file as well).

Every child runs under its own time limit (--limit seconds); if one is killed or fails, nothing
else is started.

    python tools/soft_bench.py [--trials 32768] [--repeats 5] [--rounds 3] [--libs a.so,b.so] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "m-mimo-ofdm-with-nonlinear-pa-sim_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = ("2", "paper")
ITERS = [0, 1, 2, 3, 4]


def child(a):
    import _engine
    import bench
    out = {}
    for w in WORKLOADS:
        eng = bench.make_engine(0, w, "f64")
        pt = eng._point
        rho_max = 32.0 * pt.avg_symbol_power / (4.0 * 10 ** (pt.snr_db / 10))  # Link.soft's default range
        err, _, _ = eng.run(7, 0, a.trials, ITERS)
        err_s, _, soft, _, _ = eng.soft(7, 0, a.trials, ITERS, rho_max)
        assert list(err) == list(err_s)  # the same trials, the same counts
        plain_ms, soft_ms = [], []
        for _ in range(a.repeats):
            eng.run(7, 0, a.trials, ITERS)
            plain_ms.append(eng.kernel_ms)
            eng.soft(7, 0, a.trials, ITERS, rho_max)
            soft_ms.append(eng.kernel_ms)
        st = _engine.SoftStats(soft, rho_max, eng.constel_size, a.trials)
        out[w] = dict(describe=eng.describe(), plain_ms=plain_ms, soft_ms=soft_ms, rho_max=rho_max,
                      ber=st.ber().tolist(), gmi=st.gmi().tolist(), clamped=st.clamped().tolist(),
                      negatives_equal_errors=bool(list(soft[:, :128].sum(axis=1)) == list(err)))
        eng.close()
    print("SOFT_BENCH_CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trials", type=int, default=32768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--libs", type=str, default="", help="comma-separated library paths (default: the built one)")
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one GPU child process [s]")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    libs = [os.path.abspath(p) for p in a.libs.split(",") if p] or [None]
    res = {str(lib): {w: dict(plain_ms=[], soft_ms=[]) for w in WORKLOADS} for lib in libs}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--trials", str(a.trials), "--repeats", str(a.repeats)]
    for _ in range(a.rounds):
        for lib in libs:
            env = dict(os.environ)
            if lib:
                env["MIMO_LIB"] = lib
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit, env=env)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"a GPU step ran into its limit of {a.limit:.0f} s")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("SOFT_BENCH_CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"a GPU step failed (exit status {r.returncode})")
            c = json.loads(line[0][len("SOFT_BENCH_CHILD "):])
            for w in WORKLOADS:
                for k in ("describe", "rho_max", "ber", "gmi", "clamped", "negatives_equal_errors"):
                    res[str(lib)][w][k] = c[w][k]
                res[str(lib)][w]["plain_ms"] += c[w]["plain_ms"]
                res[str(lib)][w]["soft_ms"] += c[w]["soft_ms"]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for lib in res:
        for w in WORKLOADS:
            d = res[lib][w]
            per = 1024.0 / a.trials
            d.update(plain_ms_per_1024=med(d["plain_ms"]) * per, soft_ms_per_1024=med(d["soft_ms"]) * per,
                     ratio=med(d["soft_ms"]) / med(d["plain_ms"]),
                     plain_spread=(max(d["plain_ms"]) - min(d["plain_ms"])) / med(d["plain_ms"]),
                     soft_spread=(max(d["soft_ms"]) - min(d["soft_ms"])) / med(d["soft_ms"]))
    s = json.dumps(dict(trials=a.trials, repeats=a.repeats, rounds=a.rounds, libs=res))
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
