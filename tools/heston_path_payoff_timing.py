#!/usr/bin/env python3
"""Device time of the Heston path-payoff kernels (heston_path_kernel, heston_qmc_path_kernel: arithmetic Asian, geometric Asian, extrema)
against the European kernels on the same paths (heston_kernel, heston_qmc_kernel of the same construction), by the library's own
launch timer (olmc_profile_enable / olmc_kernel_time: device events around each launch); the blocking price_asian call against the
route it replaces (simulate_paths to the host, then NumPy) by wall clock; and the scatter of the price over 16 scrambles against 16
Philox seeds.  All in one session, the calls of one comparison interleaved rep by rep.

    python tools/heston_path_payoff_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per kernel and configuration: the median (ms) and the extremes (ms_min, ms_max) over --reps timed launches (one warm-up
launch each first), and `vs_european`, the median over the European kernel's on the same paths."""
import argparse
import json
import math
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import optionslab_amd as ol  # noqa: E402
from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
MODEL = (2.0, 0.04, 0.3, -0.7, 0.04)             # kappa theta sigma_v rho v0: the project's usual
UP = 120.0
CONFIGS = [(1 << 14, 252), (1 << 17, 252), (1 << 14, 1024)]
FAMILIES = [("asian_arithmetic", _hip.PATH_ASIAN_ARITHMETIC, 0.0), ("asian_geometric", _hip.PATH_ASIAN_GEOMETRIC, 0.0),
            ("extrema_up_out", _hip.BARRIER_KINDS["up-and-out"], UP)]


def summary(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def timed_kernels(calls, reps):
    """calls: {name: launch}; every launch once to warm up, then rep by rep in turn: {name: summary}."""
    for call in calls.values():
        call()
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            _hip.profile_reset()
            call()
            n, t = _hip.kernel_time()
            assert n == 1, n
            ms[name].append(t)
    return {name: summary(v) for name, v in ms.items()}


def timed_wall(calls, reps):
    """The same for blocking calls by the host clock (each returns with its result on the host)."""
    for call in calls.values():
        call()
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    return {name: summary(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        p = ol.HestonPricer(*MODEL)
    _hip.profile_enable(True)
    for N, n in CONFIGS:
        sv, sh = sobol_tables(2 * n, 1, N)
        for antithetic in (False, True):
            calls = {"european": lambda N=N, n=n, antithetic=antithetic: _hip.heston(S, K, T, R, Q, True, *MODEL, N, n, 1, antithetic)}
            for name, payoff, level in FAMILIES:
                calls[name] = (lambda payoff=payoff, level=level, N=N, n=n, antithetic=antithetic:
                               _hip.heston_path_payoff(S, K, T, R, Q, True, *MODEL, payoff, level, N, n, 1, antithetic))
            got = timed_kernels(calls, a.reps)
            for name, t in got.items():
                emit(dict(kernel="heston_kernel" if name == "european" else "heston_path_kernel", payoff=name, paths="philox", antithetic=antithetic,
                          points=N, steps=n, vs_european=t["ms"] / got["european"]["ms"], **t))
            for bridge in (True, False):
                calls = {"european": lambda N=N, sv=sv, sh=sh, bridge=bridge, antithetic=antithetic:
                         _hip.heston_qmc(S, K, T, R, Q, True, *MODEL, N, sv, sh, bridge, antithetic)}
                for name, payoff, level in FAMILIES:
                    calls[name] = (lambda payoff=payoff, level=level, N=N, sv=sv, sh=sh, bridge=bridge, antithetic=antithetic:
                                   _hip.heston_qmc_path_payoff(S, K, T, R, Q, True, *MODEL, payoff, level, N, sv, sh, bridge, antithetic))
                got = timed_kernels(calls, a.reps)
                for name, t in got.items():
                    emit(dict(kernel="heston_qmc_kernel" if name == "european" else "heston_qmc_path_kernel", payoff=name,
                              paths="bridge" if bridge else "sequential", antithetic=antithetic, points=N, steps=n,
                              vs_european=t["ms"] / got["european"]["ms"], **t))
    _hip.profile_enable(False)

    # the blocking call against the route it replaces: both path matrices to the host, NumPy on the spot matrix
    disc = math.exp(-R * T)

    def matrix_route(N, n, **kw):
        spot, _var = p.simulate_paths(S, T, R, Q, N, n, 1, **kw)
        return disc * np.mean(np.maximum(np.mean(spot[:, 1:], axis=1) - K, 0))

    for N, n in CONFIGS:
        for label, kw in (("philox", dict()), ("bridge", dict(method="qmc"))):
            sobol_tables(2 * n, 1, N)                                    # the tables' own cost (cached per seed) stays out of both
            got = timed_wall({"price_asian": lambda N=N, n=n, kw=kw: p.price_asian(S, K, T, R, Q, "call", "arithmetic", N, n, 1, **kw),
                              "simulate_paths_numpy": lambda N=N, n=n, kw=kw: matrix_route(N, n, **kw)}, max(3, a.reps // 2))
            for name, t in got.items():
                emit(dict(call=name, clock="host wall", paths=label, points=N, steps=n, vs_fused=t["ms"] / got["price_asian"]["ms"], **t))

    # what the bridge buys for a path-dependent payoff: the scatter of the price over 16 scrambles and over 16 Philox seeds
    N, n = 1 << 14, 252
    for name, price in (("asian_arithmetic", lambda **kw: p.price_asian(S, K, T, R, Q, "call", "arithmetic", N, n, **kw)),
                        ("barrier_up_out", lambda **kw: p.price_barrier(S, K, T, R, UP, Q, "call", "up-and-out", N, n, **kw))):
        pseudo = [float(price(seed=1000 + s)) for s in range(16)]
        row = dict(scatter=name, points=N, steps=n, seeds=16, mean_philox=float(np.mean(pseudo)), sd_philox=float(np.std(pseudo, ddof=1)))
        for construction in ("bridge", "sequential"):
            qmc = [float(price(seed=s, method="qmc", path_construction=construction)) for s in range(16)]
            row["mean_" + construction] = float(np.mean(qmc))
            row["sd_" + construction] = float(np.std(qmc, ddof=1))
            row["philox_over_" + construction] = row["sd_philox"] / row["sd_" + construction]
        emit(row)
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
