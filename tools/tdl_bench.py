"""Cost of the TDL channel: HIP-event time of the Rayleigh trial kernel, of the trial kernel of a TDL
engine (the table instance reading the channel bank) and of the TDL generator kernel that fills the
bank, at BASELINE config 2 (A 64, S 1024, F 2048) and at the paper geometry (A 64, S 2048, F 4096),
float64, 64-QAM, CNC iterations 0-4, per 1,024 trials, with profiles of 8 and of 32 taps
(utilities.exp_pdp(L, 4, 3 dB)), and with the bank buffer of a launch at MIMO_BANK_BUFFER_BYTES and
lowered to 256 MiB (the environment variable of the same name lowers it).  From the times: the bytes
per second the generator writes (16 n_ant n_sub_carr per trial) and the trial kernel reads (twice
that: pass 1 and the array pass).

Per library and round one child process: per workload a warm-up call of every engine, then --repeats
rounds of calls in which the Rayleigh engine and every TDL setting take turns.  With several --libs
(A/B builds of the generator, e.g. -DMIMO_TDL_W_LDS=1) the libraries alternate round by round, so
that they share the machine's drift.  Prints one JSON line (--out writes it to a file as well).

Every child runs under its own time limit (--limit seconds); if one is killed or fails, nothing
else is started.

    python tools/tdl_bench.py [--trials 4096] [--repeats 5] [--rounds 3] [--libs a.so,b.so] [--out FILE]
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
TAPS = (8, 32)
BUFFERS = {"full": None, "256MiB": 256 << 20}


def tdl_engine(w, n_taps):
    """The workload's system (bench.WORKLOADS) on the TDL channel of n_taps taps."""
    import bench
    import sweep
    from utilities import ebn0_to_snr
    c = bench.WORKLOADS[w]
    link = sweep.paper_link(channel="tdl", receiver="cnc", precision="f64", device=0, n_ant=c["A"], n_sc=c["S"],
                            n_fft=c["F"], qam=c["M"], cp=c["CP"], n_err_min=10 ** 12, bits_sent_max=10 ** 15,
                            tdl=(n_taps, 4, 3.0))
    link.update_distortion(ibo_val_db=c["ibo"])
    link.set_snr(ebn0_to_snr(c["ebn0"], c["S"], c["S"], c["M"]))
    return link.engine()


def child(a):
    import _engine
    import bench
    out = {}
    for w in WORKLOADS:
        c = bench.WORKLOADS[w]
        ray = bench.make_engine(0, w, "f64")
        tdl = {L: tdl_engine(w, L) for L in TAPS}
        keys = ["L%d_%s" % (L, b) for L in TAPS for b in BUFFERS]
        res = dict(describe_rayleigh=ray.describe(), describe_tdl=tdl[TAPS[0]].describe(), rayleigh_ms=[],
                   capacity=_engine.bank_capacity(c["A"], c["S"], "f64"), bank_bytes_per_trial=16 * c["A"] * c["S"],
                   **{k + "_trial_ms": [] for k in keys}, **{k + "_gen_ms": [] for k in keys})

        def run_tdl(L, b, record):
            if BUFFERS[b] is None:
                os.environ.pop("MIMO_BANK_BUFFER_BYTES", None)
            else:
                os.environ["MIMO_BANK_BUFFER_BYTES"] = str(BUFFERS[b])
            err, _, _ = tdl[L].run(7, 0, a.trials, ITERS)
            if record:
                res["L%d_%s_trial_ms" % (L, b)].append(tdl[L].kernel_ms)
                res["L%d_%s_gen_ms" % (L, b)].append(tdl[L].chan_kernel_ms)
            return err

        ray.run(7, 0, a.trials, ITERS)
        for L in TAPS:
            errs = [run_tdl(L, b, False) for b in BUFFERS]
            assert all(list(e) == list(errs[0]) for e in errs)  # the split of a call changes no count
            res["L%d_ber" % L] = [float(x) / (a.trials * c["S"] * 6) for x in errs[0]]
        for _ in range(a.repeats):
            ray.run(7, 0, a.trials, ITERS)
            res["rayleigh_ms"].append(ray.kernel_ms)
            for L in TAPS:
                for b in BUFFERS:
                    run_tdl(L, b, True)
        os.environ.pop("MIMO_BANK_BUFFER_BYTES", None)
        for e in [ray] + list(tdl.values()):
            e.close()
        out[w] = res
    print("TDL_BENCH_CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trials", type=int, default=4096)
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
    res = {str(lib): {w: {} for w in WORKLOADS} for lib in libs}
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
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("TDL_BENCH_CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"a GPU step failed (exit status {r.returncode})")
            c = json.loads(line[0][len("TDL_BENCH_CHILD "):])
            for w in WORKLOADS:
                for k, v in c[w].items():
                    if k.endswith("_ms"):
                        res[str(lib)][w].setdefault(k, []).extend(v)
                    else:
                        res[str(lib)][w][k] = v
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    per = 1024.0 / a.trials
    for lib in res:
        for w in WORKLOADS:
            d = res[lib][w]
            bank = d["bank_bytes_per_trial"] * a.trials
            for k in [k for k in d if k.endswith("_ms")]:
                d[k[:-3] + "_ms_per_1024"] = med(d[k]) * per
                d[k[:-3] + "_spread"] = (max(d[k]) - min(d[k])) / med(d[k])
            for k in [k[:-7] for k in d if k.endswith("_gen_ms")]:
                d[k + "_gen_write_GBps"] = bank / (med(d[k + "_gen_ms"]) * 1e-3) / 1e9
                d[k + "_trial_read_GBps"] = 2 * bank / (med(d[k + "_trial_ms"]) * 1e-3) / 1e9
                d[k + "_trial_over_rayleigh"] = med(d[k + "_trial_ms"]) / med(d["rayleigh_ms"])
                d[k + "_gen_over_rayleigh"] = med(d[k + "_gen_ms"]) / med(d["rayleigh_ms"])
    s = json.dumps(dict(trials=a.trials, repeats=a.repeats, rounds=a.rounds, libs=res))
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
