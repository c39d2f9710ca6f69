#!/usr/bin/env python3
"""Device time of the fused Heston Greeks (heston_scenarios_kernel, heston_qmc_scenarios_kernel: the 14 contracts of
compute_greeks_unified as one launch of four recursions) against the literal route -- 14 launches of the one-contract kernels
(heston_kernel, heston_qmc_kernel of the same construction) at the same seed or tables -- and of a 16-scenario / 6-recursion launch
against one heston_kernel launch at equal N x n, by the library's own launch timer (olmc_profile_enable / olmc_kernel_time: device
events around each launch).  All in one session, the calls of one comparison interleaved rep by rep.

    python tools/heston_greeks_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per route and configuration: the median (ms) and the extremes (ms_min, ms_max) over --reps timed repetitions (one warm-up
each first), the launches a repetition made, and `literal_over_fused` / `vs_european`, the ratio of the medians."""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.greeks import fd_steps  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

S, K, T, R, Q, SIGMA = 100.0, 100.0, 1.0, 0.05, 0.01, 0.2
MODEL = (2.0, 0.04, 0.3, -0.7)                    # kappa theta sigma_v rho: the project's usual; v0 = sigma^2
CONFIGS = [(1 << 14, 252), (1 << 17, 252)]


def summary(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def timed_kernels(calls, reps):
    """calls: {name: (launches, call)}; every call once to warm up, then rep by rep in turn: {name: summary of the summed launch times}."""
    for _n, call in calls.values():
        call()
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, (launches, call) in calls.items():
            _hip.profile_reset()
            call()
            n, t = _hip.kernel_time()
            assert n == launches, (name, n)
            ms[name].append(t)
    return {name: dict(launches=calls[name][0], **summary(v)) for name, v in ms.items()}


def greeks_contracts():
    """(S, T, r, sigma) of the 14 evaluations, in compute_greeks_unified's call order."""
    h_S, h_v, h_r, h_T = fd_steps(S)
    return ([(S, T, R, SIGMA), (S + h_S, T, R, SIGMA), (S - h_S, T, R, SIGMA), (S, T, R, SIGMA + h_v), (S, T, R, SIGMA - h_v), (S, T - h_T, R, SIGMA),
             (S, T, R + h_r, SIGMA), (S, T, R - h_r, SIGMA)]
            + [(S + a * h_S, T, R, SIGMA + b * h_v) for a in (1, -1) for b in (1, -1)] + [(S + h_S, T - h_T, R, SIGMA), (S - h_S, T - h_T, R, SIGMA)])


def mixed_scenarios():
    """16 scenarios of 6 recursions (maturity and model bumps), spots, strikes and rates differing within a recursion."""
    kappa, theta, sigma_v, rho = MODEL
    v0 = SIGMA * SIGMA
    recursions = [(1.0, (kappa, theta, sigma_v, rho, v0)), (0.5, (kappa, theta, sigma_v, rho, v0)), (1.0, (kappa + 1.0, theta, sigma_v, rho, v0)),
                  (1.0, (kappa, 1.5 * theta, sigma_v, rho, v0)), (1.0, (kappa, theta, 1.2 * sigma_v, rho, v0)), (1.0, (kappa, theta, sigma_v, -0.5, v0))]
    return [(95.0 + i, 90.0 + 2.5 * (i % 9), recursions[i % 6][0], 0.01 * (i % 4), 0.005 * (i % 3), i % 3 != 0, *recursions[i % 6][1]) for i in range(16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    contracts = greeks_contracts()
    assert len(contracts) == 14
    mixed = mixed_scenarios()
    assert _hip.heston_scenario_layout(mixed)[0] == 6
    _hip.profile_enable(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        for N, n in CONFIGS:
            sv, sh = sobol_tables(2 * n, 1, N)
            for antithetic in (False, True):
                for paths in ("philox", "sequential", "bridge"):
                    bridge = paths == "bridge"
                    if paths == "philox":
                        one = lambda s, t, r, v: _hip.heston(s, K, t, r, Q, True, *MODEL, v * v, N, n, 1, antithetic)
                        fused = lambda: _hip.heston_greeks_fd(S, K, T, R, SIGMA, Q, True, *MODEL, N, n, 1, antithetic, True, want_evals=False)
                        many = lambda: _hip.heston_scenarios(mixed, N, n, 1, antithetic)
                    else:
                        one = lambda s, t, r, v: _hip.heston_qmc(s, K, t, r, Q, True, *MODEL, v * v, N, sv, sh, bridge, antithetic)
                        fused = lambda: _hip.heston_qmc_greeks_fd(S, K, T, R, SIGMA, Q, True, *MODEL, N, sv, sh, bridge, antithetic, True,
                                                                  want_evals=False)
                        many = lambda: _hip.heston_qmc_scenarios(mixed, N, sv, sh, bridge, antithetic)
                    got = timed_kernels({"fused": (1, fused), "literal": (14, lambda: [one(*c) for c in contracts]),
                                         "european": (1, lambda: one(S, T, R, SIGMA)), "scenarios16": (1, many)}, a.reps)
                    kernel = "heston_scenarios_kernel" if paths == "philox" else "heston_qmc_scenarios_kernel"
                    single = "heston_kernel" if paths == "philox" else "heston_qmc_kernel"
                    common = dict(paths=paths, antithetic=antithetic, points=N, steps=n)
                    emit(dict(route="fused greeks", kernel=kernel, contracts=14, recursions=4, **common, **got["fused"]))
                    emit(dict(route="literal greeks", kernel=single, contracts=14, **common, **got["literal"],
                              literal_over_fused=got["literal"]["ms"] / got["fused"]["ms"]))
                    emit(dict(route="one contract", kernel=single, contracts=1, **common, **got["european"]))
                    emit(dict(route="16 scenarios", kernel=kernel, contracts=16, recursions=6, **common, **got["scenarios16"],
                              vs_european=got["scenarios16"]["ms"] / got["european"]["ms"],
                              fused_greeks_vs_european=got["fused"]["ms"] / got["european"]["ms"]))
    _hip.profile_enable(False)
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
