#!/usr/bin/env python3
"""Device time of the local-volatility kernel (lv_price_kernel: ollv_price, include/olmc_local_vol.h) per payoff family, beside the
flat-volatility kernels of the same payoff at equal paths x steps (olmc_barrier, olmc_lookback, olmc_asian, olmc_european), by the
library's own launch timer (olmc_profile_enable / olmc_kernel_time: device events around each launch); and the implied volatilities
the Monte Carlo prices of the calibrated sample surface give back, cell by cell, against the surface that went in.  All in one
session, the calls of one comparison interleaved rep by rep.

    python tools/local_vol_timing.py [--reps 7] [--out FILE.jsonl] [--shape whole|row] [--timing-only]
    python tools/local_vol_timing.py --build-row          # compiles tools/ab/libolmc_lv_row.so (no GPU needed) and prints its path

--shape labels the lines with the table shape of the library that runs: "whole" (the product: the whole table in LDS) or "row", the
A/B build --build-row makes (-DOLMC_LV_ROW_LDS=1 with tools/local_vol_ab/ on the include path: only the date's time-blended row in LDS),
loaded through $OLMC_LIBRARY; --timing-only stops after the timing lines.  profiles/r20_local_vol.jsonl is
    python tools/local_vol_timing.py --build-row
    python tools/local_vol_timing.py --shape whole --out A
    OLMC_LIBRARY=tools/ab/libolmc_lv_row.so python tools/local_vol_timing.py --shape row --timing-only --out B       # then A followed by B
and the A/B library's results are checked by the product's own test file:
    OLMC_LIBRARY=tools/ab/libolmc_lv_row.so python -m pytest tests/test_gpu_local_vol.py -m gpu

Timing lines: one per payoff, table shape, antithetic flag and size: the median (ms) and the extremes over --reps timed launches (one
warm-up launch each first), and `vs_flat`, the median over the flat-volatility kernel's.  The table shapes are 1 x 2 (8 bytes of LDS:
the lookup's arithmetic alone), the typical 33 x 128 (17 KiB) and the caps 64 x 256 (64 KiB: two workgroups per CU), so the cost of
holding the whole table in LDS shows as the difference between them.  No time or ratio is asserted anywhere.
Implied-volatility lines: one per cell (strike, expiry) of create_sample_iv_surface(): the input volatility, the price of
DupireLocalVol.price_surface (out-of-the-money side) with its standard error, the volatility implied by it and the difference in
volatility points."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import optionslab_amd as ol  # noqa: E402
from optionslab_amd import _hip  # noqa: E402

S, K, T, R, Q, SIGMA = 100.0, 100.0, 1.0, 0.05, 0.01, 0.2
UP = 120.0
STEPS = 252
SIZES = [1 << 14, 1 << 15, 1 << 16, 1 << 17]


def table(n_t, n_x):
    """A smile around SIGMA with a skew and a term structure over x in [-0.5, 0.45], tau in [0, 1]."""
    x = np.linspace(-0.5, 0.45, n_x)[None, :]
    tau = np.arange(n_t)[:, None] / max(n_t - 1, 1)
    return SIGMA + 0.02 - 0.25 * x + 0.4 * x * x + 0.05 * tau, -0.5, 0.45, 1.0


TABLES = {"1x2": table(1, 2), "33x128": table(33, 128), "64x256": table(64, 256)}
FAMILIES = [
    ("barrier_up_out", _hip.BARRIER_KINDS["up-and-out"], UP, lambda N, a: _hip.barrier(S, K, T, R, SIGMA, Q, True, UP, 0, N, STEPS, 1, a), "olmc_barrier"),
    ("lookback_floating", _hip.LOOKBACK_FLOATING, 0.0, lambda N, a: _hip.lookback(S, K, T, R, SIGMA, Q, True, False, N, STEPS, 1, a), "olmc_lookback"),
    ("asian_arithmetic", _hip.PATH_ASIAN_ARITHMETIC, 0.0, lambda N, a: _hip.asian(S, K, T, R, SIGMA, Q, True, False, N, STEPS, 1, a), "olmc_asian"),
    ("asian_geometric", _hip.PATH_ASIAN_GEOMETRIC, 0.0, lambda N, a: _hip.asian(S, K, T, R, SIGMA, Q, True, True, N, STEPS, 1, a), "olmc_asian"),
    ("european", _hip.LV_EUROPEAN, 0.0, lambda N, a: _hip.european(S, K, T, R, SIGMA, Q, True, N, STEPS, 1, a), "olmc_european"),
]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", choices=("whole", "row"), default="whole")
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--build-row", action="store_true")
    a = ap.parse_args()
    if a.build_row:
        from optionslab_amd.build import build_variant
        print(build_variant(os.path.join(ROOT, "tools", "ab", "libolmc_lv_row.so"), defines=("OLMC_LV_ROW_LDS=1",),
                            extra_includes=(os.path.join(ROOT, "tools", "local_vol_ab"),)))
        return
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    _hip.profile_enable(True)
    for N in SIZES:
        for antithetic in (False, True):
            for name, payoff, level, flat, flat_entry in FAMILIES:
                calls = {"flat": lambda N=N, antithetic=antithetic, flat=flat: flat(N, antithetic)}
                for shape, tab in TABLES.items():
                    calls[shape] = (lambda tab=tab, payoff=payoff, level=level, N=N, antithetic=antithetic:
                                    _hip.lv_price(S, K, T, R, Q, True, tab, payoff, level, N, STEPS, 1, antithetic))
                got = timed_kernels(calls, a.reps)
                emit(dict(kernel=flat_entry, payoff=name, antithetic=antithetic, paths=N, steps=STEPS, **got["flat"]))
                for shape in TABLES:
                    emit(dict(kernel="lv_price_kernel", table_in_lds=a.shape, table=shape, payoff=name, antithetic=antithetic, paths=N, steps=STEPS,
                              vs_flat=got[shape]["ms"] / got["flat"]["ms"], **got[shape]))
    _hip.profile_enable(False)
    if a.timing_only:
        if a.out:
            out.close()
        return

    # the smile that comes back: the calibrated sample surface repriced on 2^18 antithetic paths x 200 steps, out-of-the-money side
    strikes, expiries, iv = ol.create_sample_iv_surface()
    model = ol.DupireLocalVol(r=R, q=0.0)
    model.calibrate(strikes, expiries, iv, S)
    for side, mask in (("put", strikes < S), ("call", strikes >= S)):
        ks = strikes[mask]
        prices, errors = model.price_surface(S, ks, expiries, R, 0.0, side, 1 << 18, 200, 1, True, return_error=True)
        for i, strike in enumerate(ks):
            for j, expiry in enumerate(expiries):
                row = dict(implied_vol_cell=True, strike=float(strike), expiry=float(expiry), option_type=side, input_vol=float(iv[j, np.flatnonzero(mask)[i]]),
                           price=float(prices[i, j]), std_error=float(errors[i, j]), paths=1 << 18, steps=200)
                try:
                    row["implied_vol"] = float(ol.implied_volatility(row["price"], S, float(strike), float(expiry), R, side, 0.0))
                    row["vol_points"] = 100.0 * (row["implied_vol"] - row["input_vol"])
                except ValueError as e:
                    row["implied_vol"], row["refused"] = None, str(e)
                emit(row)
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
