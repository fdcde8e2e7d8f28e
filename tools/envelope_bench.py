"""Cost of the envelope mode: HIP-event time of the envelope-instance trial kernel against the plain
trial kernel on the same engine, at BASELINE config 2 (A 64, S 1024, F 2048) and at the paper
geometry (A 64, S 2048, F 4096), float64, per 1,024 trials.

Per library and round one child process: per workload a warm-up call of each mode, then --repeats
pairs of calls, plain and envelope alternating.  With several --libs (A/B builds of the envelope
instances, e.g. -DMIMO_ENV_SUBH=4) the libraries alternate round by round, so that they share the
machine's drift.  Prints one JSON line (--out writes it to a file as well).

Every child runs under its own time limit (--limit seconds); if one is killed or fails, nothing
else is started.

    python tools/envelope_bench.py [--trials 32768] [--repeats 5] [--rounds 3] [--libs a.so,b.so] [--out FILE]
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


def child(a):
    import bench
    out = {}
    for w in WORKLOADS:
        eng = bench.make_engine(0, w, "f64")
        pt = eng._point
        ref_pow = pt.sat_pow / 10 ** (pt.ibo_db / 10)  # the nominal mean sample power
        eng.run(7, 0, a.trials, [0])
        _, _, env, _, _ = eng.envelope(7, 0, a.trials, [0], ref_pow)
        plain_ms, env_ms = [], []
        for _ in range(a.repeats):
            eng.run(7, 0, a.trials, [0])
            plain_ms.append(eng.kernel_ms)
            eng.envelope(7, 0, a.trials, [0], ref_pow)
            env_ms.append(eng.kernel_ms)
        out[w] = dict(describe=eng.describe(), plain_ms=plain_ms, env_ms=env_ms, hist_in_total=float(env[:128].sum()),
                      efficiency=float(env[257] / env[256]))
        eng.close()
    print("ENVELOPE_BENCH_CHILD " + json.dumps(out))


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
    res = {str(lib): {w: dict(plain_ms=[], env_ms=[]) for w in WORKLOADS} for lib in libs}
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
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("ENVELOPE_BENCH_CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"a GPU step failed (exit status {r.returncode})")
            c = json.loads(line[0][len("ENVELOPE_BENCH_CHILD "):])
            for w in WORKLOADS:
                res[str(lib)][w]["describe"] = c[w]["describe"]
                res[str(lib)][w]["hist_in_total"] = c[w]["hist_in_total"]
                res[str(lib)][w]["efficiency"] = c[w]["efficiency"]
                res[str(lib)][w]["plain_ms"] += c[w]["plain_ms"]
                res[str(lib)][w]["env_ms"] += c[w]["env_ms"]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for lib in res:
        for w in WORKLOADS:
            d = res[lib][w]
            per = 1024.0 / a.trials
            d.update(plain_ms_per_1024=med(d["plain_ms"]) * per, env_ms_per_1024=med(d["env_ms"]) * per,
                     ratio=med(d["env_ms"]) / med(d["plain_ms"]),
                     plain_spread=(max(d["plain_ms"]) - min(d["plain_ms"])) / med(d["plain_ms"]),
                     env_spread=(max(d["env_ms"]) - min(d["env_ms"])) / med(d["env_ms"]))
    s = json.dumps(dict(trials=a.trials, repeats=a.repeats, rounds=a.rounds, libs=res))
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
