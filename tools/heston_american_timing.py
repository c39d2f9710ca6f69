#!/usr/bin/env python3
"""Device time and prices of the American option under Heston (include/olha.h) -> profiles/r27_heston_american.jsonl.

    python tools/heston_american_timing.py [--reps 7] [--warmups 2] [--seeds 16] [--out profiles/r27_heston_american.jsonl]

Timing rows (kind = "timing"), at 50k x 50, 200k x 50 and 1M x 50, Euler Philox paths of the usual model, by device events
(olmc_profile_enable / olmc_kernel_time), median of --reps calls after --warmups calls:
    the whole call (one event pair around the path kernel and the step chain) for the (S, v) basis of degree 1, 2, 3 and for
    basis="spot" (degree 3), beside olmc_american_lsm at the equal shape in the same run;
    the path kernel alone (heston_paths_kernel, time-major, the event pair of olmc_heston_paths);
    per_date_us = (call - path kernel) / n_steps: the per-date launch, the step chain being n_steps launches;
    per_date_vs_spot = that figure relative to basis="spot"'s, the one-factor chain on the same matrix.  A date of the (S, v) chain
    moves 48 bytes per path against the one-factor chain's 32: 1.5 is the figure to compare with.
Price rows (kind = "prices"), at 50k x 50 over --seeds seeds, for the usual model and for sigma_v = 0.8: mean and scatter (standard
deviation over the seeds) of the degree-2 (S, v) price, the basis="spot" degree-3 price and the European price of the same seeds.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.0
USUAL = (2.0, 0.04, 0.3, -0.7, 0.04)
HIGH = (2.0, 0.04, 0.8, -0.7, 0.04)
SHAPES = [(50_000, 50), (200_000, 50), (1_000_000, 50)]
SPOT_DEGREE = 3


def device_ms(call, reps, warmups):
    from optionslab_amd import _hip

    for _ in range(warmups):
        call()
    ms = []
    for _ in range(reps):
        _hip.profile_reset()
        call()
        k, t = _hip.kernel_time()
        assert k == 1, k
        ms.append(t)
    return statistics.median(ms)


def timing_rows(a):
    from optionslab_amd import _hip

    _hip.profile_enable(True)
    for n_paths, n_steps in SHAPES:
        paths_ms = device_ms(lambda: _hip.heston_paths(S, T, R, Q, *USUAL, n_paths, n_steps, 1), a.reps, a.warmups)
        gbm_ms = device_ms(lambda: _hip.american_lsm(S, K, T, R, 0.2, Q, False, n_paths, n_steps, SPOT_DEGREE, 1), a.reps, a.warmups)
        calls = {("spot", SPOT_DEGREE): lambda: _hip.heston_american_lsm(S, K, T, R, Q, False, *USUAL, n_paths, n_steps, 1, SPOT_DEGREE, True)}
        for d in (1, 2, 3):
            calls["spot_variance", d] = lambda d=d: _hip.heston_american_lsm(S, K, T, R, Q, False, *USUAL, n_paths, n_steps, 1, d)
        call_ms = {key: device_ms(call, a.reps, a.warmups) for key, call in calls.items()}
        spot_per_date = (call_ms["spot", SPOT_DEGREE] - paths_ms) / n_steps
        for (basis, degree), ms in call_ms.items():
            per_date = (ms - paths_ms) / n_steps
            yield dict(kind="timing", n_paths=n_paths, n_steps=n_steps, basis=basis, poly_degree=degree, call_ms=ms, path_kernel_ms=paths_ms,
                       per_date_us=1e3 * per_date, per_date_vs_spot=per_date / spot_per_date, olmc_american_lsm_call_ms=gbm_ms, reps=a.reps,
                       warmups=a.warmups)
    _hip.profile_enable(False)


def price_rows(a):
    import numpy as np

    import optionslab_amd as ol

    n_paths, n_steps = SHAPES[0]
    for name, model in (("usual", USUAL), ("sigma_v=0.8", HIGH)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)             # Feller
            p = ol.HestonPricer(*model)
        seeds = range(1, a.seeds + 1)
        columns = {
            "spot_variance_degree_2": [float(p.price_american(S, K, T, R, Q, "put", n_paths, n_steps, 2, s)) for s in seeds],
            "spot_degree_3": [float(p.price_american(S, K, T, R, Q, "put", n_paths, n_steps, SPOT_DEGREE, s, basis="spot")) for s in seeds],
            "european": [float(p.price_monte_carlo(S, K, T, R, Q, "put", n_paths, n_steps, s)) for s in seeds],
        }
        row = dict(kind="prices", model=name, n_paths=n_paths, n_steps=n_steps, seeds=a.seeds)
        for key, xs in columns.items():
            row[key + "_mean"], row[key + "_scatter"] = float(np.mean(xs)), float(np.std(xs, ddof=1))
        diff = np.array(columns["spot_variance_degree_2"]) - np.array(columns["spot_degree_3"])
        row["state_minus_spot_mean"], row["state_minus_spot_scatter"] = float(diff.mean()), float(diff.std(ddof=1))
        yield row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_heston_american.jsonl"))
    a = ap.parse_args()
    from optionslab_amd import _hip

    info = _hip.device_info()
    rows = [dict(kind="device", name=info["name"], arch=info["arch"], compute_units=info["compute_units"])]
    for row in list(timing_rows(a)) + list(price_rows(a)):
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
