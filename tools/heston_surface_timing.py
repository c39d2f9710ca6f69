#!/usr/bin/env python3
"""Device time of the Heston surface kernels (heston_surface_kernel, heston_qmc_surface_kernel: 16 cells over 4 maturities) against the
one-contract kernels on the same paths (heston_kernel, heston_qmc_kernel of the same construction), by the library's own launch timer
(olmc_profile_enable / olmc_kernel_time: device events around each launch); the blocking 5 x 7 price_surface against the literal route,
one price_monte_carlo per cell, by wall clock; the scatter of the price over 16 scrambles against 16 Philox seeds at the at-the-money
cell of three maturities; and one calibration to quotes the model made itself.  All in one session, the calls of one comparison
interleaved rep by rep.

    python tools/heston_surface_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per kernel and configuration: the median (ms) and the extremes (ms_min, ms_max) over --reps timed launches (one warm-up
launch each first), and `vs_european`, the median over the one-contract kernel's on the same paths."""
import argparse
import json
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
from optionslab_amd.black_scholes import implied_volatility  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
MODEL = (2.0, 0.04, 0.3, -0.7, 0.04)             # kappa theta sigma_v rho v0: the project's usual
CONFIGS = [(1 << 17, 252), (1 << 14, 64)]


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

    # 1. the surface kernels against the one-contract kernels at equal N x n: 16 cells, four strikes at each of four maturities
    _hip.profile_enable(True)
    for N, n in CONFIGS:
        ks = [90.0, 100.0, 110.0, 120.0] * 4
        ms = [m for m in (n // 4, n // 2, 3 * n // 4, n) for _ in range(4)]
        sv, sh = sobol_tables(2 * n, 1, N)
        for antithetic in (False, True):
            got = timed_kernels({"european": lambda: _hip.heston(S, K, T, R, Q, True, *MODEL, N, n, 1, antithetic),
                                 "surface": lambda: _hip.heston_surface(S, T, R, Q, True, *MODEL, ks, ms, N, n, 1, antithetic)}, a.reps)
            for name, t in got.items():
                emit(dict(kernel="heston_kernel" if name == "european" else "heston_surface_kernel", cells=1 if name == "european" else 16,
                          paths="philox", antithetic=antithetic, points=N, steps=n, vs_european=t["ms"] / got["european"]["ms"], **t))
            for bridge in (True, False):
                got = timed_kernels({"european": lambda: _hip.heston_qmc(S, K, T, R, Q, True, *MODEL, N, sv, sh, bridge, antithetic),
                                     "surface": lambda: _hip.heston_qmc_surface(S, T, R, Q, True, *MODEL, ks, ms, N, sv, sh, bridge, antithetic)},
                                    a.reps)
                for name, t in got.items():
                    emit(dict(kernel="heston_qmc_kernel" if name == "european" else "heston_qmc_surface_kernel",
                              cells=1 if name == "european" else 16, paths="bridge" if bridge else "sequential", antithetic=antithetic, points=N,
                              steps=n, vs_european=t["ms"] / got["european"]["ms"], **t))
    _hip.profile_enable(False)

    # 2. the blocking 5 x 7 surface against the literal route: one price_monte_carlo per cell, each on its own grid of m steps
    strikes = (80.0, 90.0, 100.0, 110.0, 120.0)
    for N, n in CONFIGS:
        steps = [n * j // 7 for j in range(1, 8)] if n % 7 == 0 else [n * j // 8 for j in range(1, 8)] + [n]
        steps = sorted(set(steps))[-7:]
        maturities = [T * m / n for m in steps]
        for label, kw in (("philox", dict()), ("bridge", dict(method="qmc"))):
            for m in steps:
                sobol_tables(2 * m, 1, N)                                # the tables' own cost (cached per seed) stays out of both
            sobol_tables(2 * n, 1, N)

            def literal():
                return [[p.price_monte_carlo(S, k, t, R, Q, "call", N, m, 1, **kw) for t, m in zip(maturities, steps)] for k in strikes]

            got = timed_wall({"price_surface": lambda: p.price_surface(S, strikes, maturities, R, Q, "call", N, n, 1, **kw),
                              "price_monte_carlo_x35": literal}, max(3, a.reps // 2))
            for name, t in got.items():
                emit(dict(call=name, clock="host wall", paths=label, points=N, steps=n, cell_steps=steps,
                          vs_surface=t["ms"] / got["price_surface"]["ms"], **t))

    # 3. what Sobol points buy at an intermediate date of the full-horizon construction: the scatter of the at-the-money price over 16
    #    scrambles and over 16 Philox seeds
    N, n = 1 << 14, 64
    maturities = (0.25, 0.5, 1.0)
    pseudo = np.array([p.price_surface(S, (K,), maturities, R, Q, "call", N, n, 1000 + s)[0] for s in range(16)])
    qmc = {c: np.array([p.price_surface(S, (K,), maturities, R, Q, "call", N, n, s, method="qmc", path_construction=c)[0] for s in range(16)])
           for c in ("bridge", "sequential")}
    for j, t in enumerate(maturities):
        row = dict(scatter="atm_call", maturity=t, points=N, steps=n, seeds=16, mean_philox=float(np.mean(pseudo[:, j])),
                   sd_philox=float(np.std(pseudo[:, j], ddof=1)))
        for c in ("bridge", "sequential"):
            row["mean_" + c] = float(np.mean(qmc[c][:, j]))
            row["sd_" + c] = float(np.std(qmc[c][:, j], ddof=1))
            row["philox_over_" + c] = row["sd_philox"] / row["sd_" + c]
        emit(row)

    # 4. one calibration from the reference's default start to quotes the usual model made itself (same seed and settings)
    strikes, settings = (90.0, 100.0, 110.0), dict(n_paths=1 << 14, n_steps=64, seed=7)
    prices = p.price_surface(S, strikes, maturities, R, Q, "call", method="qmc", **settings)
    ivs = [[implied_volatility(float(prices[i, j]), S, strikes[i], maturities[j], R, "call", Q) for j in range(3)] for i in range(3)]
    market = dict(spot=S, strikes=strikes, maturities=maturities, market_ivs=ivs, r=R, q=Q)
    start = ol.heston.calibration_objective(market, **settings)((2.0, 0.04, 0.3, -0.5, 0.04))
    t0 = time.perf_counter()
    fitted = ol.calibrate_heston(market, **settings)
    emit(dict(calibration="quotes of the usual model at 3 x 3 cells", truth=list(MODEL), start_error=start, seconds=time.perf_counter() - t0,
              fitted=[fitted.kappa, fitted.theta, fitted.sigma_v, fitted.rho, fitted.v0], error=fitted.calibration_error,
              surfaces=fitted.calibration_evals, **settings))
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
