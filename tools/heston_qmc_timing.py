#!/usr/bin/env python3
"""Device time of the Heston Sobol kernels (heston_qmc_kernel, heston_qmc_paths_kernel; bridge and sequential) against the Philox
ones (heston_kernel, heston_paths_kernel) at equal points x steps, by the library's own launch timer (olmc_profile_enable /
olmc_kernel_time: device events around each launch), all in one session.

    python tools/heston_qmc_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per kernel and configuration: the median (ms) and the extremes (ms_min, ms_max) over --reps timed launches (one
warm-up launch first), and `vs_philox`, the median over the Philox kernel's at the same size."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
MODEL = (2.0, 0.04, 0.3, -0.7, 0.04)             # kappa theta sigma_v rho v0: the project's usual
CONFIGS = [(1 << 14, 252), (1 << 17, 252), (1 << 20, 50), (1 << 14, 1024)]


def timed(call, reps):
    call()
    ms = []
    for _ in range(reps):
        _hip.profile_reset()
        call()
        n, t = _hip.kernel_time()
        assert n == 1, n
        ms.append(t)
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.profile_enable(True)
    out = open(a.out, "w") if a.out else sys.stdout
    for N, n in CONFIGS:
        sv, sh = sobol_tables(2 * n, 1, N)
        for antithetic in (False, True):
            base = timed(lambda: _hip.heston(S, K, T, R, Q, True, *MODEL, N, n, 1, antithetic), a.reps)
            rows = [dict(kernel="heston_kernel", paths="philox", antithetic=antithetic, points=N, steps=n, **base)]
            for bridge in (True, False):
                t = timed(lambda: _hip.heston_qmc(S, K, T, R, Q, True, *MODEL, N, sv, sh, bridge, antithetic), a.reps)
                rows.append(dict(kernel="heston_qmc_kernel", paths="bridge" if bridge else "sequential", antithetic=antithetic, points=N, steps=n,
                                 vs_philox=t["ms"] / base["ms"], **t))
            for row in rows:
                out.write(json.dumps(row) + "\n")
                out.flush()
        base = timed(lambda: _hip.heston_paths(S, T, R, Q, *MODEL, N, n, 1), a.reps)
        rows = [dict(kernel="heston_paths_kernel", paths="philox", layout="time-major", points=N, steps=n, **base)]
        for bridge in (True, False):
            t = timed(lambda: _hip.heston_qmc_paths(S, T, R, Q, *MODEL, N, sv, sh, bridge), a.reps)
            rows.append(dict(kernel="heston_qmc_paths_kernel", paths="bridge" if bridge else "sequential", layout="time-major", points=N, steps=n,
                             vs_philox=t["ms"] / base["ms"], **t))
        for row in rows:
            out.write(json.dumps(row) + "\n")
            out.flush()
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
