"""Cost of the coded mode: HIP-event time of the coded-instance trial kernel against the plain trial
kernel on the same engine, and of the LDPC decoder kernel, at BASELINE config 2 (A 64, S 1024,
F 2048) and at the paper geometry (A 64, S 2048, F 4096), float64, 64-QAM, CNC iterations 0-4 all
recorded, per 1,024 trials.  The code is utilities.qc_ldpc_code(512, 3, 6) with 10 decoder
iterations: N 3,072, 2 codewords per trial and counter index at config 2 and 4 at the paper geometry.

Per library and round one child process: per workload a warm-up call of each mode, then --repeats
pairs of calls, plain and coded alternating.  With several --libs (A/B builds of the coded
instances, e.g. -DMIMO_CODED_W64_2048=2) the libraries alternate round by round, so that they share
the machine's drift.  Prints one JSON line (--out writes it to a file as well).

Every child runs under its own time limit (--limit seconds); if one is killed or fails, nothing
else is started.

    python tools/coded_bench.py [--trials 32768] [--repeats 5] [--rounds 3] [--libs a.so,b.so] [--out FILE]
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
    from utilities import qc_ldpc_code
    code = qc_ldpc_code(512, 3, 6, n_dec_iters=10)
    out = {}
    for w in WORKLOADS:
        eng = bench.make_engine(0, w, "f64")
        pt = eng._point
        rho_max = 32.0 * pt.avg_symbol_power / (4.0 * 10 ** (pt.snr_db / 10))  # Link.coded's default range
        n_cw = eng.coded_codewords(code)
        err, _, _ = eng.run(7, 0, a.trials, ITERS)
        err_c, _, coded, _, _ = eng.coded(7, 0, a.trials, ITERS, code, rho_max)
        assert list(err) == list(err_c)  # the same trials, the same counts
        plain_ms, coded_ms, decode_ms = [], [], []
        for _ in range(a.repeats):
            eng.run(7, 0, a.trials, ITERS)
            plain_ms.append(eng.kernel_ms)
            eng.coded(7, 0, a.trials, ITERS, code, rho_max)
            coded_ms.append(eng.kernel_ms)
            decode_ms.append(eng.decode_kernel_ms)
        st = _engine.CodedStats(coded, a.trials * n_cw, code.n_bits)
        out[w] = dict(describe=eng.describe(), plain_ms=plain_ms, coded_ms=coded_ms, decode_ms=decode_ms,
                      rho_max=rho_max, n_cw=n_cw, raw_ber=st.raw_ber().tolist(), ber=st.ber().tolist(),
                      fer=st.fer().tolist(), syndrome_rate=st.syndrome_rate().tolist(),
                      raw_equals_errors=bool(list(coded[:, 0]) == list(err)))  # every position is decoded here
        eng.close()
    print("CODED_BENCH_CHILD " + json.dumps(out))


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
    series = ("plain_ms", "coded_ms", "decode_ms")
    res = {str(lib): {w: {k: [] for k in series} for w in WORKLOADS} for lib in libs}
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
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CODED_BENCH_CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"a GPU step failed (exit status {r.returncode})")
            c = json.loads(line[0][len("CODED_BENCH_CHILD "):])
            for w in WORKLOADS:
                for k in ("describe", "rho_max", "n_cw", "raw_ber", "ber", "fer", "syndrome_rate", "raw_equals_errors"):
                    res[str(lib)][w][k] = c[w][k]
                for k in series:
                    res[str(lib)][w][k] += c[w][k]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for lib in res:
        for w in WORKLOADS:
            d = res[lib][w]
            per = 1024.0 / a.trials
            d.update(plain_ms_per_1024=med(d["plain_ms"]) * per, coded_ms_per_1024=med(d["coded_ms"]) * per,
                     decode_ms_per_1024=med(d["decode_ms"]) * per, ratio=med(d["coded_ms"]) / med(d["plain_ms"]),
                     decode_over_plain=med(d["decode_ms"]) / med(d["plain_ms"]),
                     **{k[:-3] + "_spread": (max(d[k]) - min(d[k])) / med(d[k]) for k in series})
    s = json.dumps(dict(trials=a.trials, repeats=a.repeats, rounds=a.rounds, libs=res))
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
