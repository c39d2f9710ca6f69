#!/usr/bin/env python3
"""The autocallable and the cliquet under Heston on the device, measured in one session:

1. the time of every structured-product kernel (Euler / QE, Philox / Sobol, plain / antithetic) by the library's own launch timer
   (olmc_profile_enable / olmc_kernel_time: device events around each launch), median of --reps launches interleaved rep by rep with its
   neighbour at equal N x n: heston_path_kernel's / heston_qmc_path_kernel's extrema family (a floating lookback) for Euler,
   heston_qe_surface_kernel / heston_qe_qmc_surface_kernel (one cell at the last step) for QE -- `vs_neighbour` is the ratio of medians;
2. the only route without these kernels: simulate_paths' two matrices to the host plus the NumPy payoff, by the host clock, median of 3,
   against the fused call by the same clock;
3. the price scatter over 16 scrambles against 16 Philox seeds.

    python tools/heston_structured_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per measurement; times are the median (ms) and the extremes (ms_min, ms_max)."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import optionslab_amd as ol  # noqa: E402
from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402
from oracle import numpy_reference as orc  # noqa: E402
from tests import heston_qe_reference as qe  # noqa: E402
from tools.heston_surface_timing import timed_kernels, timed_wall  # noqa: E402

S, T, R, Q = 100.0, 1.0, 0.05, 0.01
CONFIGS = [(1 << 17, 12, 3, 12), (1 << 17, 252, 21, 12)]          # points, steps, observation_freq, n_periods
AUTOCALL = (1.0, 0.9, 0.10, 0.8)
CLIQUET = (0.05, -0.05, 0.30, 0.0)
MODEL = qe.FELLER_VIOLATED


def pricer(model):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return ol.HestonPricer(*model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    m = MODEL
    # 1. kernel times against the neighbouring kernels at equal N x n
    _hip.profile_enable(True)
    for N, n, f, periods in CONFIGS:
        sv, sh = sobol_tables(2 * n, 1, N)
        for anti in (False, True):
            groups = {
                ("euler", "philox"): {
                    "neighbour": lambda: _hip.heston_path_payoff(S, S, T, R, Q, True, *m, _hip.LOOKBACK_FLOATING, 0.0, N, n, 1, anti),
                    "autocallable": lambda: _hip.heston_autocallable(S, T, R, Q, *m, *AUTOCALL, f, N, n, 1, anti),
                    "cliquet": lambda: _hip.heston_cliquet(S, T, R, Q, *m, *CLIQUET, periods, N, n, 1, anti)},
                ("qe", "philox"): {
                    "neighbour": lambda: _hip.heston_qe_surface(S, T, R, Q, True, *m, [S], [n], N, n, 1, anti),
                    "autocallable": lambda: _hip.heston_autocallable(S, T, R, Q, *m, *AUTOCALL, f, N, n, 1, anti, qe=True),
                    "cliquet": lambda: _hip.heston_cliquet(S, T, R, Q, *m, *CLIQUET, periods, N, n, 1, anti, qe=True)},
                ("qe", "sequential"): {
                    "neighbour": lambda: _hip.heston_qe_qmc_surface(S, T, R, Q, True, *m, [S], [n], N, sv, sh, False, anti),
                    "autocallable": lambda: _hip.heston_autocallable_qmc(S, T, R, Q, *m, *AUTOCALL, f, N, sv, sh, False, anti, qe=True),
                    "cliquet": lambda: _hip.heston_cliquet_qmc(S, T, R, Q, *m, *CLIQUET, periods, N, sv, sh, False, anti, qe=True)},
            }
            for bridge in (False, True):
                groups[("euler", "bridge" if bridge else "sequential")] = {
                    "neighbour": lambda b=bridge: _hip.heston_qmc_path_payoff(S, S, T, R, Q, True, *m, _hip.LOOKBACK_FLOATING, 0.0, N, sv, sh, b, anti),
                    "autocallable": lambda b=bridge: _hip.heston_autocallable_qmc(S, T, R, Q, *m, *AUTOCALL, f, N, sv, sh, b, anti),
                    "cliquet": lambda b=bridge: _hip.heston_cliquet_qmc(S, T, R, Q, *m, *CLIQUET, periods, N, sv, sh, b, anti)}
            for (scheme, paths), calls in groups.items():
                got = timed_kernels(calls, a.reps)
                for name, t in got.items():
                    emit(dict(kernel_time=name, scheme=scheme, paths=paths, antithetic=anti, points=N, steps=n, observation_freq=f,
                              n_periods=periods, model=list(m), vs_neighbour=t["ms"] / got["neighbour"]["ms"], **t))
    _hip.profile_enable(False)

    # 2. the route through the path matrices, by the host clock
    p = pricer(m)
    for N, n, f, periods in CONFIGS:
        for scheme in ("euler", "qe"):
            def matrix_autocall():
                spot = p.simulate_paths(S, T, R, Q, N, n, 1, scheme=scheme)[0]
                return orc.autocallable_from_paths(spot, S, T, R, f, AUTOCALL[0], AUTOCALL[1], AUTOCALL[2], AUTOCALL[3])

            def matrix_cliquet():
                spot = p.simulate_paths(S, T, R, Q, N, n, 1, scheme=scheme)[0]
                return orc.cliquet_from_paths(spot, S, T, R, periods, *CLIQUET)

            got = timed_wall({"matrix_autocallable": matrix_autocall, "matrix_cliquet": matrix_cliquet,
                              "fused_autocallable": lambda: p.price_autocallable(S, T, R, Q, *AUTOCALL, f, N, n, 1, scheme=scheme),
                              "fused_cliquet": lambda: p.price_cliquet(S, T, R, Q, *CLIQUET, periods, N, n, 1, scheme=scheme)}, 3)
            for product in ("autocallable", "cliquet"):
                emit(dict(host_clock=product, scheme=scheme, points=N, steps=n, matrix=got["matrix_" + product], fused=got["fused_" + product],
                          matrix_over_fused=got["matrix_" + product]["ms"] / got["fused_" + product]["ms"]))

    # 3. the scatter over 16 scrambles against 16 Philox seeds at 2^14 x 12, both products, both schemes
    N, n, f, periods = 1 << 14, 12, 3, 12
    for scheme in ("euler", "qe"):
        for product, price in (("autocallable", lambda **kw: p.price_autocallable(S, T, R, Q, *AUTOCALL, f, N, n, scheme=scheme, **kw)),
                               ("cliquet", lambda **kw: p.price_cliquet(S, T, R, Q, *CLIQUET, periods, N, n, scheme=scheme, **kw))):
            row = dict(scatter=product, scheme=scheme, points=N, steps=n, seeds=16, model=list(m))
            pseudo = np.array([price(seed=1000 + s) for s in range(16)])
            row.update(mean_philox=float(pseudo.mean()), sd_philox=float(pseudo.std(ddof=1)))
            for construction in ("sequential",) if scheme == "qe" else ("sequential", "bridge"):
                sobol = np.array([price(seed=s, method="qmc", path_construction=construction) for s in range(16)])
                row["mean_" + construction] = float(sobol.mean())
                row["sd_" + construction] = float(sobol.std(ddof=1))
                row["philox_over_" + construction] = float(pseudo.std(ddof=1) / sobol.std(ddof=1))
            emit(row)
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
