#!/usr/bin/env python3
"""Device time of the American option (LSM) on Sobol paths (olmc_american_lsm_qmc) against Philox paths (olmc_american_lsm), and of
the Sobol path-matrix kernel (lsm_qmc_paths_kernel) against the Philox one (lsm_paths_kernel).

    python tools/lsm_qmc_timing.py calls [--reps 7] > calls.jsonl
        whole calls by device events (olmc_profile_enable / olmc_kernel_time: one event pair around the path kernel and the step chain),
        median of --reps calls after one warm-up call
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_I -- python tools/lsm_qmc_timing.py launch --config I [--reps 5]
        the calls of configuration I, untimed, for the kernel trace (one process per configuration: the stats are per kernel name)
    python tools/lsm_qmc_timing.py merge --calls calls.jsonl --stats DIR_0 DIR_1 ... [--reps 5] --out profiles/r08_lsm_qmc_timing.jsonl
        one JSON line per configuration and path source: the whole call, the path kernel and the step chain per call, in ms."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, K, T, R, SIG, Q, DEG = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0, 3
# (points, dates, Sobol constructions priced)
CONFIGS = [(1 << 20, 50, ("bridge", "sequential")), (1 << 17, 252, ("bridge", "sequential")), (1 << 14, 1024, ("bridge",))]


def calls_of(cfg):
    """[(label, call)]: the Philox price and one Sobol price per construction, at the same points and dates."""
    from optionslab_amd import _hip
    from optionslab_amd.monte_carlo import sobol_tables

    N, n, constructions = CONFIGS[cfg]
    sv, sh = sobol_tables(n, 1, N)
    out = [("philox", lambda: _hip.american_lsm(S, K, T, R, SIG, Q, False, N, n, DEG, 1))]
    for c in constructions:
        out.append((c, lambda c=c: _hip.american_lsm_qmc(S, K, T, R, SIG, Q, False, N, sv, sh, c == "bridge", DEG)))
    return out


def cmd_calls(a):
    from optionslab_amd import _hip

    _hip.profile_enable(True)
    for cfg, (N, n, _) in enumerate(CONFIGS):
        for label, call in calls_of(cfg):
            call()
            ms = []
            for _ in range(a.reps):
                _hip.profile_reset()
                call()
                k, t = _hip.kernel_time()
                assert k == 1, k
                ms.append(t)
            print(json.dumps(dict(config=cfg, paths=label, points=N, dates=n, call_ms=statistics.median(ms), reps=a.reps)), flush=True)


def cmd_launch(a):
    for label, call in calls_of(a.config):
        for _ in range(a.reps + 1):                 # one warm-up call each
            call()


def kernel_stats(d):
    """{kernel name: (calls, total ns)} from rocprofv3's *kernel_stats.csv under d."""
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel_stats.csv under {d}"
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def cmd_merge(a):
    calls = [json.loads(line) for line in open(a.calls) if line.startswith("{")]
    rows = []
    for cfg, d in enumerate(a.stats):
        st = kernel_stats(d)
        per_call = a.reps + 1

        def ms(pred):
            return sum(t for name, (_, t) in st.items() if pred(name)) / per_call / 1e6

        N, n, constructions = CONFIGS[cfg]
        chain = ms(lambda name: "lsm_step_kernel" in name) / (1 + len(constructions))    # every call runs the same chain
        for c in calls:
            if c["config"] != cfg:
                continue
            if c["paths"] == "philox":
                kernel, path_ms = "lsm_paths_kernel", ms(lambda name: "lsm_paths_kernel" in name and "qmc" not in name)
            else:
                tags = ("<true, false>", "ILb1ELb0E") if c["paths"] == "bridge" else ("<false, false>", "ILb0ELb0E")   # demangled or not
                kernel = "lsm_qmc_paths_kernel"
                path_ms = ms(lambda name, tags=tags: "lsm_qmc_paths_kernel" in name and any(t in name for t in tags))
            rows.append(dict(c, path_kernel=kernel, path_kernel_ms=path_ms, step_chain_ms=chain, step_launches=n))
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("calls")
    p.add_argument("--reps", type=int, default=7)
    p = sub.add_parser("launch")
    p.add_argument("--config", type=int, required=True)
    p.add_argument("--reps", type=int, default=5)
    p = sub.add_parser("merge")
    p.add_argument("--calls", required=True)
    p.add_argument("--stats", nargs="+", required=True)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", required=True)
    a = ap.parse_args()
    {"calls": cmd_calls, "launch": cmd_launch, "merge": cmd_merge}[a.cmd](a)


if __name__ == "__main__":
    main()
