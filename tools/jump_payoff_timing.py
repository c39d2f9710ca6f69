#!/usr/bin/env python3
"""Device time of the jump-diffusion path kernels (jump_path_kernel, jump_surface_kernel, jump_product_kernel: include/olmc_jump.h)
against the European kernel on the same paths (jump_kernel), by the library's own launch timer (olmc_profile_enable /
olmc_kernel_time: device events around each launch); the antithetic launch against two plain ones; the blocking calls against the
route they replace (simulate_paths to the host, then NumPy) by wall clock; and, over 16 seeds, the scatter of the antithetic price
against the plain price at the equal sample count.  All in one session, the calls of one comparison interleaved rep by rep.

    python tools/jump_payoff_timing.py [--reps 7] [--out profiles/r23_jump_payoffs.jsonl]

Models: the tests' Merton M0 and Kou K0 (lambda dt ~ 2e-3 .. 4e-3 at 252 steps: a lane in a few hundred jumps), and for each a heavy
intensity, lambda dt = 3 at 252 steps with small jumps (nearly every lane jumps at every step; Kou draws one fp64 log per jump).
One JSON line per kernel and configuration: the median (ms) and the extremes (ms_min, ms_max) over --reps timed launches (one warm-up
launch each first), and `vs_european`, the median over jump_kernel's at the same shape and model."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import optionslab_amd as ol  # noqa: E402
from optionslab_amd import _hip  # noqa: E402

S, K, T, R, Q, SIGMA = 100.0, 100.0, 1.0, 0.05, 0.01, 0.2
UP = 120.0
STEPS = 252
COUNTS = [1 << 14, 1 << 15, 1 << 16, 1 << 17]
# (kou, lambda_j, a1, a2, a3)
MODELS = {"merton": (False, 0.5, -0.1, 0.2, 0.0), "kou": (True, 1.0, 0.4, 10.0, 5.0),
          "merton_heavy": (False, 3.0 * STEPS, 0.0, 0.01, 0.0), "kou_heavy": (True, 3.0 * STEPS, 0.5, 200.0, 200.0)}
FAMILIES = [("european", _hip.JD_EUROPEAN, 0.0), ("asian_arithmetic", _hip.PATH_ASIAN_ARITHMETIC, 0.0),
            ("asian_geometric", _hip.PATH_ASIAN_GEOMETRIC, 0.0), ("extrema_up_out", _hip.BARRIER_KINDS["up-and-out"], UP)]
AUTOCALL, CLIQUET = (1.0, 0.8, 0.10, 0.6, 21), (0.05, -0.05, 0.30, 0.0, 12)          # the methods' defaults
CELLS = ([90.0, 100.0, 110.0] * 4, [63] * 3 + [126] * 3 + [189] * 3 + [252] * 3)


def summary(ms):
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def timed_kernels(calls, reps):
    """calls: {name: (launches per call, call)}; every call once to warm up, then rep by rep in turn: {name: summary of the device time}."""
    for _k, call in calls.values():
        call()
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, (launches, call) in calls.items():
            _hip.profile_reset()
            call()
            n, t = _hip.kernel_time()
            assert n == launches, (name, n)
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


def pricer(model):
    return ol.KouJumpDiffusion(*model[1:]) if model[0] else ol.MertonJumpDiffusion(*model[1:4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        row = {k: float("%.5g" % v) if isinstance(v, float) else v for k, v in row.items()}      # five digits: the spread is in the third
        out.write(json.dumps(row) + "\n")
        out.flush()

    n = STEPS
    _hip.profile_enable(True)
    for label, model in MODELS.items():
        for N in COUNTS:
            calls = {"jump_kernel": (1, lambda N=N, model=model: _hip.jump_diffusion(S, K, T, R, SIGMA, Q, True, *model, N, n, 1))}
            for antithetic in (False, True):
                tag = "/anti" if antithetic else ""
                for name, payoff, level in FAMILIES:
                    calls["jump_path_kernel/" + name + tag] = (1, lambda payoff=payoff, level=level, N=N, model=model, antithetic=antithetic:
                                                               _hip.jd_price(S, K, T, R, SIGMA, Q, True, model, payoff, level, N, n, 1, antithetic))
                calls["jump_surface_kernel/12_cells" + tag] = (1, lambda N=N, model=model, antithetic=antithetic:
                                                               _hip.jd_surface_prices(S, T, R, SIGMA, Q, True, model, *CELLS, N, n, 1, antithetic))
                calls["jump_product_kernel/autocallable" + tag] = (1, lambda N=N, model=model, antithetic=antithetic:
                                                                   _hip.jd_autocallable(S, T, R, SIGMA, Q, model, *AUTOCALL, N, n, 1, antithetic))
                calls["jump_product_kernel/cliquet" + tag] = (1, lambda N=N, model=model, antithetic=antithetic:
                                                              _hip.jd_cliquet(S, T, R, SIGMA, Q, model, *CLIQUET, N, n, 1, antithetic))
            # the antithetic launch's rival at the equal sample count: two plain launches (paths [0, N) and [N, 2N))
            for name, payoff, level in FAMILIES:
                calls["two_plain_launches/" + name] = (2, lambda payoff=payoff, level=level, N=N, model=model:
                                                       [_hip.jd_price(S, K, T, R, SIGMA, Q, True, model, payoff, level, N, n, 1, False, o) for o in (0, N)])
            got = timed_kernels(calls, a.reps)
            base = got["jump_kernel"]["ms"]
            for name, t in got.items():
                row = dict(kernel=name.split("/")[0], what=name, model=label, paths=N, steps=n, vs_european=t["ms"] / base, **t)
                if name.startswith("two_plain_launches/"):
                    row["antithetic_over_two_plain"] = got["jump_path_kernel/" + name.split("/")[1] + "/anti"]["ms"] / t["ms"]
                emit(row)
    _hip.profile_enable(False)

    # the blocking calls against the route they replace: the path matrix to the host, NumPy on it
    disc = math.exp(-R * T)
    for label in ("merton", "kou_heavy"):
        p = pricer(MODELS[label])
        for N in COUNTS:
            def asian_route(N=N):
                spot = p.simulate_paths(S, T, R, SIGMA, Q, N, n, 1)
                return disc * np.mean(np.maximum(np.mean(spot[:, 1:], axis=1) - K, 0))

            def barrier_route(N=N):
                spot = p.simulate_paths(S, T, R, SIGMA, Q, N, n, 1)
                alive = np.max(spot, axis=1) < UP
                return disc * np.mean(np.where(alive, np.maximum(spot[:, -1] - K, 0), 0.0))

            got = timed_wall({"price_asian": lambda N=N: p.price_asian(S, K, T, R, SIGMA, Q, "call", "arithmetic", N, n, 1),
                              "simulate_paths_numpy_asian": asian_route,
                              "price_barrier": lambda N=N: p.price_barrier(S, K, T, R, SIGMA, UP, Q, "call", "up-and-out", N, n, 1),
                              "simulate_paths_numpy_barrier": barrier_route}, max(3, a.reps // 2))
            for name, t in got.items():
                fused = got["price_asian" if name.endswith("asian") else "price_barrier"]["ms"]
                emit(dict(call=name, clock="host wall", model=label, paths=N, steps=n, vs_fused=t["ms"] / fused, **t))

    # what the mirror buys: over 16 seeds, the antithetic price on N paths against the plain price on 2 N paths (equal sample count)
    N = 1 << 14
    for label in ("merton", "kou", "kou_heavy"):
        model = MODELS[label]
        for name, payoff, level in FAMILIES:
            plain = [_hip.jd_price(S, K, T, R, SIGMA, Q, True, model, payoff, level, 2 * N, n, 1000 + s, False).price for s in range(16)]
            anti = [_hip.jd_price(S, K, T, R, SIGMA, Q, True, model, payoff, level, N, n, 1000 + s, True).price for s in range(16)]
            emit(dict(scatter=name, model=label, samples=2 * N, steps=n, seeds=16, mean_plain=float(np.mean(plain)), sd_plain=float(np.std(plain, ddof=1)),
                      mean_antithetic=float(np.mean(anti)), sd_antithetic=float(np.std(anti, ddof=1)),
                      plain_over_antithetic=float(np.std(plain, ddof=1) / np.std(anti, ddof=1))))
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
