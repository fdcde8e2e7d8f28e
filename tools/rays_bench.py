"""Cost of the ray-cluster channel: HIP-event time of the generator kernel of a TDL engine on a
power-delay profile (mimo_engine_set_tdl) and on ray-cluster profiles at the same delays
(mimo_engine_set_rays), and of the trial kernel behind each, at BASELINE config 2 (A 64, S 1024,
F 2048) and at the paper geometry (A 64, S 2048, F 4096), float64, 64-QAM, CNC iterations 0-4, per
1,024 trials.  Profiles: utilities.exp_pdp(L, 4, 3 dB) with L = 8 and 32 taps; the ray-cluster ones
put utilities.ring_clusters' clusters of 1 ray, of 20 rays and of 1024 / L rays (R = 1,024, the most
a profile holds) on those taps.

Per library and round one child process: per workload a warm-up call of every engine, then --repeats
rounds of calls in which the settings take turns.  With several --libs (A/B builds of the generator,
e.g. -DMIMO_TDL_W_LDS_MAX_F=2048) the libraries alternate round by round, so that they share the
machine's drift.  Prints one JSON line (--out writes it to a file as well).

Every child runs under its own time limit (--limit seconds); if one is killed or fails, nothing
else is started.

    python tools/rays_bench.py [--trials 4096] [--repeats 5] [--rounds 3] [--libs a.so,b.so] [--out FILE]
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
RAYS_MAX = 1024


def settings(n_taps):
    """name -> rays per cluster (None: the power-delay profile itself)."""
    return {"tdl": None, "rays1": 1, "rays20": 20, "rays%d" % (RAYS_MAX // n_taps): RAYS_MAX // n_taps}


def engine(w, n_taps, per_cluster):
    """The workload's system (bench.WORKLOADS) on the profile of n_taps taps, as taps or as clusters."""
    import bench
    import sweep
    from utilities import ebn0_to_snr
    c = bench.WORKLOADS[w]
    link = sweep.paper_link(channel="tdl" if per_cluster is None else "rays", receiver="cnc", precision="f64", device=0,
                            n_ant=c["A"], n_sc=c["S"], n_fft=c["F"], qam=c["M"], cp=c["CP"], n_err_min=10 ** 12,
                            bits_sent_max=10 ** 15, tdl=(n_taps, 4, 3.0), rays=(None, per_cluster, 5.0, 300.0, None))
    link.update_distortion(ibo_val_db=c["ibo"])
    link.set_snr(ebn0_to_snr(c["ebn0"], c["S"], c["S"], c["M"]))
    return link.engine()


def child(a):
    import bench
    out = {}
    for w in WORKLOADS:
        c = bench.WORKLOADS[w]
        eng = {"L%d_%s" % (L, k): engine(w, L, m) for L in TAPS for k, m in settings(L).items()}
        res = dict(describe=next(iter(eng.values())).describe(), bank_bytes_per_trial=16 * c["A"] * c["S"],
                   **{k + "_trial_ms": [] for k in eng}, **{k + "_gen_ms": [] for k in eng})
        for k, e in eng.items():  # warm-up
            err, _, _ = e.run(7, 0, a.trials, ITERS)
            res[k + "_ber"] = [float(x) / (a.trials * c["S"] * 6) for x in err]
        for _ in range(a.repeats):
            for k, e in eng.items():
                e.run(7, 0, a.trials, ITERS)
                res[k + "_trial_ms"].append(e.kernel_ms)
                res[k + "_gen_ms"].append(e.chan_kernel_ms)
        for e in eng.values():
            e.close()
        out[w] = res
    print("RAYS_BENCH_CHILD " + json.dumps(out))


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
    for rnd in range(a.rounds):
        for lib in libs:
            env = dict(os.environ)
            if lib:
                env["MIMO_LIB"] = lib
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit, env=env)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"a GPU step ran into its limit of {a.limit:.0f} s")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RAYS_BENCH_CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"a GPU step failed (exit status {r.returncode})")
            c = json.loads(line[0][len("RAYS_BENCH_CHILD "):])
            sys.stderr.write("round %d, %s: done\n" % (rnd + 1, os.path.basename(lib) if lib else "the built library"))
            sys.stderr.flush()
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
            for k in [k for k in d if k.endswith("_ms")]:
                d[k[:-3] + "_ms_per_1024"] = med(d[k]) * per
                d[k[:-3] + "_spread"] = (max(d[k]) - min(d[k])) / med(d[k])
            for L in TAPS:
                for k in settings(L):
                    if k != "tdl":
                        d["L%d_%s_gen_over_tdl" % (L, k)] = med(d["L%d_%s_gen_ms" % (L, k)]) / med(d["L%d_tdl_gen_ms" % L])
    s = json.dumps(dict(trials=a.trials, repeats=a.repeats, rounds=a.rounds, libs=res))
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
