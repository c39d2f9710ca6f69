#!/usr/bin/env python3
"""Device time and price scatter of SABR on scrambled-Sobol points (include/olmc_sabr_qmc.h), by the library's own launch timer
(olmc_profile_enable / olmc_kernel_time: device events around each launch), all in one process, the calls of one comparison
interleaved rep by rep.

    python tools/sabr_qmc_timing.py [--reps 7] [--out profiles/r29_sabr_qmc.jsonl]

Timing lines (2^14 x 252 and 2^17 x 252; one model per kernel kind: beta = 1, 0.5, 0 and 0.7): one per kernel, payoff, construction and
antithetic flag with the median (ms) and the extremes over --reps timed launches after one warm-up each:
  sabr_qmc_price_kernel    codes 8, 6, 4, 0 (European, arithmetic Asian, floating lookback, up-and-out); beside it in the same run
                           sabr_price_kernel (olsb_price, Philox) and heston_qmc_path_kernel (same payoff, construction and flag; codes
                           6, 4, 0) at the equal shape, with the ratios `vs_philox` and `vs_heston_qmc`;
  sabr_qmc_paths_kernel    both layouts (the plain leg);
  sabr_qmc_surface_kernel  16 cells over 4 maturities.
Scatter lines (2^12 x 64 and 2^14 x 252, the `half` model, codes 8, 6, 4, 0, both constructions): the standard deviation of the price
over 16 scrambles (seeds 0 .. 15) and over 16 Philox seeds (1000 .. 1015), their ratio, and from the times of the same run
`time_to_equal_error`: the device time Philox needs for the Sobol run's error -- ratio^2 times the paths at sabr_price_kernel's time per
path at 2^17 x steps -- over the Sobol kernel's time; above 1 the Sobol construction is cheaper per unit of error.  No time or ratio
is asserted here."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optionslab_amd import _hip  # noqa: E402
from optionslab_amd.monte_carlo import sobol_tables  # noqa: E402

F, K, T, R, Q = 100.0, 100.0, 1.0, 0.03, 0.0
UP = 112.0
HESTON = (2.0, 0.04, 0.3, -0.7, 0.04)
# alpha beta rho nu: tests/sabr_oracle.py's models that do not absorb, and a beta = 0 one
MODELS = {"lognormal": (0.25, 1.0, -0.4, 0.5), "half": (2.5, 0.5, -0.3, 0.4), "normal": (20.0, 0.0, -0.3, 0.4), "general": (0.9, 0.7, 0.2, 0.6)}
STEPS = 252
SIZES = [1 << 14, 1 << 17]
PAYOFFS = [("european", 8, 0.0), ("asian_arithmetic", 6, 0.0), ("lookback_floating", 4, 0.0), ("barrier_up_out", 0, UP)]
SCATTER_MODEL = "half"
SCATTER_SHAPES = [(1 << 12, 64), (1 << 14, 252)]


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
    a = ap.parse_args()
    if not _hip.hip_available():
        raise SystemExit("no HIP device: nothing is measured without one")
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    sobol_ms, philox_ms_per_path = {}, {}           # (code, bridge, N, steps) -> ms; (code, steps) -> ms per path at 2^17: the scatter model's
    _hip.profile_enable(True)
    for N in SIZES:
        sv, shift = sobol_tables(2 * STEPS, 1, N)
        for model_name, model in MODELS.items():
            for name, code, level in PAYOFFS:
                for anti in (False, True):
                    calls = {"philox": lambda: _hip.sabr_price(F, K, T, R, True, model, code, level, N, STEPS, 1, anti)}
                    for bridge in (False, True):
                        calls["sabr", bridge] = lambda bridge=bridge: _hip.sabrq_price(F, K, T, R, True, model, code, level, N, sv, shift, bridge, anti)
                        if code != 8:
                            calls["heston", bridge] = (lambda bridge=bridge:
                                                       _hip.heston_qmc_path_payoff(F, K, T, R, Q, True, *HESTON, code, level, N, sv, shift, bridge, anti))
                    got = timed_kernels(calls, a.reps)
                    emit(dict(kernel="sabr_price_kernel", model=model_name, beta=model[1], payoff=name, antithetic=anti, paths=N, steps=STEPS,
                              **got["philox"]))
                    if not anti and model_name == SCATTER_MODEL:
                        philox_ms_per_path[code, STEPS] = got["philox"]["ms"] / N
                    for bridge in (False, True):
                        row = dict(kernel="sabr_qmc_price_kernel", model=model_name, beta=model[1], payoff=name,
                                   construction="bridge" if bridge else "sequential", antithetic=anti, paths=N, steps=STEPS,
                                   vs_philox=got["sabr", bridge]["ms"] / got["philox"]["ms"], **got["sabr", bridge])
                        if code != 8:
                            emit(dict(kernel="heston_qmc_path_kernel", payoff=name, construction=row["construction"], antithetic=anti, paths=N,
                                      steps=STEPS, beside=model_name, **got["heston", bridge]))
                            row["vs_heston_qmc"] = got["sabr", bridge]["ms"] / got["heston", bridge]["ms"]
                        emit(row)
                        if not anti and model_name == SCATTER_MODEL:
                            sobol_ms[code, bridge, N, STEPS] = got["sabr", bridge]["ms"]
            cells = ([90.0, 100.0, 110.0, 120.0] * 4, [m for m in (63, 126, 189, 252) for _ in range(4)])
            calls = {}
            for bridge in (False, True):
                for path_major in (False, True):
                    calls["paths", bridge, path_major] = (lambda bridge=bridge, path_major=path_major:
                                                          _hip.sabrq_paths(F, T, model, N, sv, shift, bridge, False, path_major))
                for anti in (False, True):
                    calls["surface", bridge, anti] = (lambda bridge=bridge, anti=anti:
                                                      _hip.sabrq_surface_prices(F, T, R, True, model, *cells, N, sv, shift, bridge, anti))
            got = timed_kernels(calls, a.reps)
            for (kind, bridge, flag), s in got.items():
                extra = dict(path_major=flag) if kind == "paths" else dict(antithetic=flag, cells=16)
                emit(dict(kernel=f"sabr_qmc_{kind}_kernel", model=model_name, beta=model[1], construction="bridge" if bridge else "sequential", paths=N,
                          steps=STEPS, **extra, **s))

    # the scatter: 16 scrambles against 16 Philox seeds, and what it is worth in device time
    model = MODELS[SCATTER_MODEL]
    for N, n in SCATTER_SHAPES:
        for name, code, level in PAYOFFS:
            philox = [_hip.sabr_price(F, K, T, R, True, model, code, level, N, n, 1000 + s, False).price for s in range(16)]
            if (code, n) not in philox_ms_per_path:                                 # 2^17 x 64: the Philox kernel's time per path at this step count
                big = timed_kernels({"philox": lambda: _hip.sabr_price(F, K, T, R, True, model, code, level, 1 << 17, n, 1, False)}, a.reps)
                philox_ms_per_path[code, n] = big["philox"]["ms"] / (1 << 17)
            for bridge in (False, True):
                sobol = [_hip.sabrq_price(F, K, T, R, True, model, code, level, N, *sobol_tables(2 * n, s, N), bridge, False).price for s in range(16)]
                if (code, bridge, N, n) not in sobol_ms:
                    sv, shift = sobol_tables(2 * n, 1, N)
                    one = timed_kernels({"sabr": lambda: _hip.sabrq_price(F, K, T, R, True, model, code, level, N, sv, shift, bridge, False)}, a.reps)
                    sobol_ms[code, bridge, N, n] = one["sabr"]["ms"]
                ratio = float(np.std(philox, ddof=1) / np.std(sobol, ddof=1))
                philox_equal_ms = ratio * ratio * N * philox_ms_per_path[code, n]
                emit(dict(scatter=True, model=SCATTER_MODEL, payoff=name, code=code, construction="bridge" if bridge else "sequential", paths=N, steps=n,
                          seeds=16, philox_std=float(np.std(philox, ddof=1)), sobol_std=float(np.std(sobol, ddof=1)), ratio=ratio,
                          paths_of_equal_error=ratio * ratio * N, philox_ms_at_equal_error=philox_equal_ms, sobol_ms=sobol_ms[code, bridge, N, n],
                          time_to_equal_error=philox_equal_ms / sobol_ms[code, bridge, N, n]))
    _hip.profile_enable(False)
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
