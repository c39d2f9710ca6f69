#!/usr/bin/env python3
"""Device time of the fused Sobol-path Greeks (olmc_asian_qmc_greeks_fd / olmc_extrema_qmc_greeks_fd: the 14 contracts of second-order
compute_greeks_unified in ONE launch) against the 14 literal launches of olmc_asian_qmc / olmc_extrema_qmc it replaces, by the
library's own launch timer (olmc_profile_enable / olmc_kernel_time).

    python tools/qmc_greeks_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per configuration: fused_ms = the median over --reps fused launches, literal_ms = the median over --reps rounds of the
SUM of the 14 literal launches (one warm-up of each first), ratio = literal_ms / fused_ms; same_bits = how many of the 14 evaluations
came out with the bits of their own launch (sum and sum of squares)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.exotic import reference_barrier_level  # noqa: E402
from optionslab_amd.greeks import fd_steps  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0


def contracts():
    """(S, T, r, sigma) of the 14 second-order evaluations, in the ABI's order."""
    h_S, h_v, h_r, h_T = fd_steps(S)
    return [(S, T, R, SIG), (S + h_S, T, R, SIG), (S - h_S, T, R, SIG), (S, T, R, SIG + h_v), (S, T, R, SIG - h_v), (S, T - h_T, R, SIG),
            (S, T, R + h_r, SIG), (S, T, R - h_r, SIG), (S + h_S, T, R, SIG + h_v), (S + h_S, T, R, SIG - h_v), (S - h_S, T, R, SIG + h_v),
            (S - h_S, T, R, SIG - h_v), (S + h_S, T - h_T, R, SIG), (S - h_S, T - h_T, R, SIG)]


def timed(call, reps, launches):
    out = call()
    ms = []
    for _ in range(reps):
        _hip.profile_reset()
        call()
        n, t = _hip.kernel_time()
        assert n == launches, (n, launches)
        ms.append(t)
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _hip.profile_enable(True)
    up = reference_barrier_level(S, 120.0, "up-and-out")
    families = {   # name: (fused(N, sv, sh, bridge), alone(contract, N, sv, sh, bridge))
        "asian_arithmetic": (lambda N, sv, sh, b: _hip.asian_qmc_greeks_fd(S, K, T, R, SIG, Q, True, False, N, sv, sh, b, False, True),
                             lambda c, N, sv, sh, b: _hip.asian_qmc(c[0], K, c[1], c[2], c[3], Q, True, False, N, sv, sh, b)),
        "asian_geometric": (lambda N, sv, sh, b: _hip.asian_qmc_greeks_fd(S, K, T, R, SIG, Q, True, True, N, sv, sh, b, False, True),
                            lambda c, N, sv, sh, b: _hip.asian_qmc(c[0], K, c[1], c[2], c[3], Q, True, True, N, sv, sh, b)),
        "barrier_up_out": (lambda N, sv, sh, b: _hip.extrema_qmc_greeks_fd(S, K, T, R, SIG, Q, True, 0, up, N, sv, sh, b, False, True),
                           lambda c, N, sv, sh, b: _hip.extrema_qmc(c[0], K, c[1], c[2], c[3], Q, True, 0, up, N, sv, sh, b)),
        "lookback_floating": (lambda N, sv, sh, b: _hip.extrema_qmc_greeks_fd(S, K, T, R, SIG, Q, True, _hip.LOOKBACK_FLOATING, 0.0, N, sv, sh, b,
                                                                               False, True),
                              lambda c, N, sv, sh, b: _hip.extrema_qmc(c[0], K, c[1], c[2], c[3], Q, True, _hip.LOOKBACK_FLOATING, 0.0, N, sv,
                                                                       sh, b)),
        "lookback_fixed": (lambda N, sv, sh, b: _hip.extrema_qmc_greeks_fd(S, K, T, R, SIG, Q, True, _hip.LOOKBACK_FIXED, 0.0, N, sv, sh, b,
                                                                            False, True),
                           lambda c, N, sv, sh, b: _hip.extrema_qmc(c[0], K, c[1], c[2], c[3], Q, True, _hip.LOOKBACK_FIXED, 0.0, N, sv, sh, b)),
    }
    rows = []
    configs = [(1 << 14, 252), (1 << 17, 252), (1 << 17, 1024)]
    cs = contracts()
    for N, n in configs:
        sv, sh = sobol_tables(n, 1, N)
        for name, (fused, alone) in families.items():
            for bridge in (True, False):
                fused_ms, (_vals, evals) = timed(lambda: fused(N, sv, sh, bridge), a.reps, 1)
                literal_ms, stats = timed(lambda: [alone(c, N, sv, sh, bridge) for c in cs], a.reps, len(cs))
                same = sum(e.n == s.n and e.sum == s.sum and e.sumsq == s.sumsq for e, s in zip(evals, stats))
                worst = max(abs(e.sum - s.sum) / max(abs(s.sum), 1e-300) for e, s in zip(evals, stats))
                rows.append(dict(kernel="qmc_path_greeks", payoff=name, construction="bridge" if bridge else "sequential", points=N, dates=n,
                                 contracts=len(cs), fused_ms=fused_ms, literal_ms=literal_ms, ratio=literal_ms / fused_ms, same_bits=same,
                                 worst_rel_sum=worst))
                print(json.dumps(rows[-1]), file=sys.stderr)
    out = open(a.out, "w") if a.out else sys.stdout
    for row in rows:
        out.write(json.dumps(row) + "\n")
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
