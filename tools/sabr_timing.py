#!/usr/bin/env python3
"""Device time and prices of the SABR path kernels (include/olmc_sabr.h) -> profiles/r28_sabr.jsonl.

    python tools/sabr_timing.py [--reps 7] [--warmups 2] [--seeds 16] [--out profiles/r28_sabr.jsonl]

Timing rows by device events (olmc_profile_enable / olmc_kernel_time), median of --reps calls after --warmups calls, at 2^14 x 252 and
2^17 x 252, F = 100, T = 1, r = 0.03, alpha = 0.2 F^(1 - beta), rho = -0.3, nu = 0.4:
    kind = "price"    every family of sabr_price_kernel (European, arithmetic and geometric Asian, extrema: the floating lookback) for beta
                      in {1, 0.5, 0, 0.7}, plain and antithetic, beside heston_kernel (European) or heston_path_kernel (the same payoff)
                      at the same shape in the same run: vs_heston = sabr_ms / heston_ms;
    kind = "surface"  twelve cells (four strikes at steps 63, 126, 252) of sabr_surface_kernel beside heston_surface_kernel.
Host rows (kind = "asian-vs-numpy", wall clock, median of --reps): the blocking SABRModel.price_asian against simulate_paths plus the
NumPy mean and payoff of the same paths.
Price rows (kind = "hagan"), 2^17 x 64 over --seeds seeds: at (rho, nu) = (-0.3, 0.4) and (-0.7, 0.8), beta in {1, 0.5, 0}, K in
{80, 100, 120}, the mean call price over the seeds, the standard error of that mean (the seeds' scatter / sqrt(seeds)), Hagan's price
and the gap in those standard errors.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, K, T, R = 100.0, 100.0, 1.0, 0.03
HESTON = (2.0, 0.04, 0.3, -0.7, 0.04)
SHAPES = [(1 << 14, 252), (1 << 17, 252)]
BETAS = (1.0, 0.5, 0.0, 0.7)
FAMILIES = (("european", 8), ("asian-arithmetic", 6), ("asian-geometric", 7), ("lookback-floating", 4))
CELL_STRIKES, CELL_STEPS = [90.0, 100.0, 110.0, 120.0] * 3, [63] * 4 + [126] * 4 + [252] * 4
HAGAN_SETS = ((-0.3, 0.4), (-0.7, 0.8))
HAGAN_SHAPE = (1 << 17, 64)


def model(beta, rho=-0.3, nu=0.4):
    return (0.2 * F ** (1 - beta), beta, rho, nu)


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


def wall_ms(call, reps, warmups):
    for _ in range(warmups):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def timing_rows(a):
    from optionslab_amd import _hip

    _hip.profile_enable(True)
    for n_paths, n_steps in SHAPES:
        common = dict(n_paths=n_paths, n_steps=n_steps, reps=a.reps, warmups=a.warmups)
        for anti in (False, True):
            for family, code in FAMILIES:
                if code == 8:
                    beside, heston = "heston_kernel", lambda: _hip.heston(F, K, T, R, 0.0, True, *HESTON, n_paths, n_steps, 1, anti)
                else:
                    beside, heston = "heston_path_kernel", lambda: _hip.heston_path_payoff(F, K, T, R, 0.0, True, *HESTON, code, 0.0, n_paths, n_steps, 1, anti)
                heston_ms = device_ms(heston, a.reps, a.warmups)
                for beta in BETAS:
                    ms = device_ms(lambda: _hip.sabr_price(F, K, T, R, True, model(beta), code, 0.0, n_paths, n_steps, 1, anti), a.reps, a.warmups)
                    yield dict(kind="price", family=family, beta=beta, antithetic=anti, sabr_ms=ms, beside=beside, heston_ms=heston_ms,
                               vs_heston=ms / heston_ms, **common)
            heston_ms = device_ms(lambda: _hip.heston_surface(F, T, R, 0.0, True, *HESTON, CELL_STRIKES, CELL_STEPS, n_paths, n_steps, 1, anti), a.reps, a.warmups)
            for beta in BETAS:
                ms = device_ms(lambda: _hip.sabr_surface_prices(F, T, R, True, model(beta), CELL_STRIKES, CELL_STEPS, n_paths, n_steps, 1, anti), a.reps,
                               a.warmups)
                yield dict(kind="surface", cells=len(CELL_STRIKES), beta=beta, antithetic=anti, sabr_ms=ms, beside="heston_surface_kernel",
                           heston_ms=heston_ms, vs_heston=ms / heston_ms, **common)
    _hip.profile_enable(False)


def host_rows(a):
    import numpy as np

    import optionslab_amd as ol

    for n_paths, n_steps in SHAPES:
        for beta in (1.0, 0.5):
            m = ol.SABRModel(*model(beta))

            def by_numpy():
                forward, _vol = m.simulate_paths(F, T, n_paths, n_steps, 1)
                return np.exp(-R * T) * np.maximum(forward[:, 1:].mean(axis=1) - K, 0.0).mean()

            one_launch = wall_ms(lambda: m.price_asian(F, K, T, R, n_paths=n_paths, n_steps=n_steps, seed=1), a.reps, a.warmups)
            matrix = wall_ms(by_numpy, a.reps, a.warmups)
            yield dict(kind="asian-vs-numpy", beta=beta, n_paths=n_paths, n_steps=n_steps, price_asian_ms=one_launch, paths_plus_numpy_ms=matrix,
                       speedup=matrix / one_launch, price=float(m.price_asian(F, K, T, R, n_paths=n_paths, n_steps=n_steps, seed=1)), numpy_price=float(by_numpy()),
                       reps=a.reps, warmups=a.warmups)


def hagan_rows(a):
    import numpy as np

    import optionslab_amd as ol
    from optionslab_amd import _hip

    n_paths, n_steps = HAGAN_SHAPE
    strikes = [80.0, 100.0, 120.0]
    for rho, nu in HAGAN_SETS:
        for beta in (1.0, 0.5, 0.0):
            params = model(beta, rho, nu)
            prices = np.array([[st.price for st in _hip.sabr_surface_prices(F, T, R, True, params, strikes, [n_steps] * 3, n_paths, n_steps, seed)]
                               for seed in range(1, a.seeds + 1)])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                hagan = [float(ol.SABRModel(*params).price(F, k, T, R, "call")) for k in strikes]
            for j, k in enumerate(strikes):
                mean, se = float(prices[:, j].mean()), float(prices[:, j].std(ddof=1) / np.sqrt(a.seeds))
                yield dict(kind="hagan", alpha=params[0], beta=beta, rho=rho, nu=nu, K=k, n_paths=n_paths, n_steps=n_steps, seeds=a.seeds, mc_mean=mean,
                           mc_se=se, hagan=hagan[j], gap=mean - hagan[j], gap_in_se=(mean - hagan[j]) / se)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_sabr.jsonl"))
    a = ap.parse_args()
    from optionslab_amd import _hip

    info = _hip.device_info()
    rows = [dict(kind="device", name=info["name"], arch=info["arch"], compute_units=info["compute_units"])]
    for row in list(timing_rows(a)) + list(host_rows(a)) + list(hagan_rows(a)):
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
