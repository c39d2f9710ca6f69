#!/usr/bin/env python3
"""Device time of the Sobol path-payoff kernels (olmc_asian_qmc / olmc_extrema_qmc / olmc_autocallable_qmc / olmc_cliquet_qmc) next to
the European Sobol kernel and the pseudo-random Asian, autocallable and cliquet kernels, by the library's own launch timer
(olmc_profile_enable / olmc_kernel_time: events around each launch).

    python tools/qmc_path_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per configuration: the median (ms) and the extremes (ms_min, ms_max) over --reps timed launches (one warm-up launch
first), in ms."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.exotic import reference_barrier_level  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0
AUTOCALL = (1.0, 0.8, 0.10, 0.6, 21)             # autocall and coupon levels, coupon rate, knock-in level, observation frequency: the class defaults
CLIQUET = (0.05, -0.05, 0.30, 0.0, 12)           # local cap / floor, global cap / floor, periods: the class defaults


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
    rows = []
    payoffs = {
        "asian_arithmetic": lambda N, sv, sh, b: _hip.asian_qmc(S, K, T, R, SIG, Q, True, False, N, sv, sh, b),
        "asian_geometric": lambda N, sv, sh, b: _hip.asian_qmc(S, K, T, R, SIG, Q, True, True, N, sv, sh, b),
        "barrier_up_out": lambda N, sv, sh, b: _hip.extrema_qmc(S, K, T, R, SIG, Q, True, 0, reference_barrier_level(S, 120.0, "up-and-out"),
                                                                N, sv, sh, b),
        "lookback_floating": lambda N, sv, sh, b: _hip.extrema_qmc(S, K, T, R, SIG, Q, True, _hip.LOOKBACK_FLOATING, 0.0, N, sv, sh, b),
        "lookback_fixed": lambda N, sv, sh, b: _hip.extrema_qmc(S, K, T, R, SIG, Q, True, _hip.LOOKBACK_FIXED, 0.0, N, sv, sh, b),
        "autocallable": lambda N, sv, sh, b: _hip.autocallable_qmc(S, T, R, SIG, Q, *AUTOCALL, N, sv, sh, b),
        "cliquet": lambda N, sv, sh, b: _hip.cliquet_qmc(S, T, R, SIG, Q, *CLIQUET, N, sv, sh, b),
    }
    configs = [(1 << p, 252) for p in (14, 17, 20)] + [(1 << 17, 1024)]
    for N, n in configs:
        sv, sh = sobol_tables(n, 1, N)
        for name, f in payoffs.items():
            for bridge in (True, False):
                rows.append(dict(kernel="qmc_path", payoff=name, construction="bridge" if bridge else "sequential", points=N, dates=n,
                                 **timed(lambda: f(N, sv, sh, bridge), a.reps)))
        if n == 252:
            rows.append(dict(kernel="european_qmc", points=N, dates=n,
                             **timed(lambda: _hip.european_qmc(S, K, T, R, SIG, Q, True, N, sv, sh), a.reps)))
    # the pseudo-random Asian at the path counts that reach the Sobol bridge's error at 2^14 (36-46x smaller RMSE: ~1000-2000x the paths)
    for N in (1 << 14, 1 << 20, 1 << 24):
        for geo in (False, True):
            rows.append(dict(kernel="asian_pseudo", payoff="asian_geometric" if geo else "asian_arithmetic", points=N, dates=252,
                             **timed(lambda: _hip.asian(S, K, T, R, SIG, Q, True, geo, N, 252, 1), a.reps)))
    # the pseudo-random autocallable / cliquet at 2^14 paths and at the count that reaches the Sobol bridge's error at 2^14 points
    # (standard deviations 2.2x / 3.6x smaller on the CPU oracle: ratio^2 times the paths)
    for N in (1 << 14, round(2.2**2 * (1 << 14))):
        rows.append(dict(kernel="autocallable_pseudo", payoff="autocallable", points=N, dates=252,
                         **timed(lambda: _hip.autocallable(S, T, R, SIG, Q, *AUTOCALL, N, 252, 1), a.reps)))
    for N in (1 << 14, round(3.6**2 * (1 << 14))):
        rows.append(dict(kernel="cliquet_pseudo", payoff="cliquet", points=N, dates=252,
                         **timed(lambda: _hip.cliquet(S, T, R, SIG, Q, *CLIQUET, N, 252, 1), a.reps)))
    out = open(a.out, "w") if a.out else sys.stdout
    for row in rows:
        out.write(json.dumps(row) + "\n")
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
