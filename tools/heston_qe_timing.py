#!/usr/bin/env python3
"""Heston's quadratic-exponential scheme on the device, measured: the time of each QE kernel against its Euler counterpart of the same
build (the Euler kernels are the parent commit's, untouched) by the library's own launch timer (olmc_profile_enable / olmc_kernel_time:
device events around each launch); the bias of both schemes against the characteristic-function price as the steps grow, and the step
count at which Euler comes inside 3 standard errors of 2^20 paths; the worst deviation of the device's paths from the NumPy restatement
(tests/heston_qe_reference.py) and the share of steps on the exponential branch; and the price scatter of 16 scrambles against 16
Philox seeds.  All in one session, the calls of one comparison interleaved rep by rep.

    python tools/heston_qe_timing.py [--reps 7] [--out FILE.jsonl]

One JSON line per measurement; times are the median (ms) and the extremes (ms_min, ms_max) over --reps timed launches after one warm-up
launch each, `vs_euler` the median over the Euler kernel's at the same N x n."""
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
from oracle import philox_oracle  # noqa: E402
from tests import heston_qe_reference as qe  # noqa: E402
from tools.heston_surface_timing import timed_kernels  # noqa: E402

S, T, R, Q = 100.0, 1.0, 0.05, 0.0
CONFIGS = [(1 << 17, 16), (1 << 17, 64)]
BIAS_MODELS = ("feller_violated", "steep")


def pricer(model):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return ol.HestonPricer(*model)


def worst(got, want, floor):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), floor)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()

    # 1. every QE kernel against its Euler counterpart at equal N x n: surfaces of 16 cells (four strikes at each of four maturities),
    #    path matrices in the reference's layout
    model = qe.FELLER_VIOLATED
    _hip.profile_enable(True)
    for N, n in CONFIGS:
        ks = [90.0, 100.0, 110.0, 120.0] * 4
        ms = [m for m in (n // 4, n // 2, 3 * n // 4, n) for _ in range(4)]
        sv, sh = sobol_tables(2 * n, 1, N)
        for antithetic in (False, True):
            pairs = {
                "philox": {"euler": lambda: _hip.heston_surface(S, T, R, Q, True, *model, ks, ms, N, n, 1, antithetic),
                           "qe": lambda: _hip.heston_qe_surface(S, T, R, Q, True, *model, ks, ms, N, n, 1, antithetic)},
                "sequential": {"euler": lambda: _hip.heston_qmc_surface(S, T, R, Q, True, *model, ks, ms, N, sv, sh, False, antithetic),
                               "qe": lambda: _hip.heston_qe_qmc_surface(S, T, R, Q, True, *model, ks, ms, N, sv, sh, False, antithetic)},
            }
            for paths, calls in pairs.items():
                got = timed_kernels(calls, a.reps)
                for scheme, t in got.items():
                    emit(dict(kernel=("heston_qe_" if scheme == "qe" else "heston_") + ("qmc_" if paths == "sequential" else "") + "surface_kernel",
                              cells=16, paths=paths, antithetic=antithetic, points=N, steps=n, model=list(model),
                              vs_euler=t["ms"] / got["euler"]["ms"], **t))
        pairs = {
            "philox": {"euler": lambda: _hip.heston_paths(S, T, R, Q, *model, N, n, 1, path_major=True),
                       "qe": lambda: _hip.heston_qe_paths(S, T, R, Q, *model, N, n, 1, path_major=True)},
            "sequential": {"euler": lambda: _hip.heston_qmc_paths(S, T, R, Q, *model, N, sv, sh, False, path_major=True),
                           "qe": lambda: _hip.heston_qe_qmc_paths(S, T, R, Q, *model, N, sv, sh, False, path_major=True)},
        }
        for paths, calls in pairs.items():
            got = timed_kernels(calls, max(3, a.reps // 2))
            for scheme, t in got.items():
                emit(dict(kernel=("heston_qe_" if scheme == "qe" else "heston_") + ("qmc_" if paths == "sequential" else "") + "paths_kernel",
                          layout="path-major", paths=paths, points=N, steps=n, model=list(model), vs_euler=t["ms"] / got["euler"]["ms"], **t))
    _hip.profile_enable(False)

    # 2. bias in standard errors of 2^20 Philox paths (seed 7) against the characteristic-function call, K = 100 and 120; the first
    #    Euler step count inside 3 standard errors at both strikes, if any up to 1024
    N = 1 << 20
    for name in BIAS_MODELS:
        model = qe.MODELS[name]
        p = pricer(model)
        anchors = {k: qe.heston_call(S, k, T, R, Q, model) for k in (100.0, 120.0)}
        euler_inside = None
        for scheme, grid in (("qe", (4, 8, 16, 64)), ("euler", (16, 32, 64, 128, 256, 512, 1024))):
            for n in grid:
                prices, errors = p.price_surface(S, (100.0, 120.0), (T,), R, Q, "call", N, n, 7, return_error=True, scheme=scheme)
                bias = [float((prices[i, 0] - anchors[k]) / errors[i, 0]) for i, k in enumerate((100.0, 120.0))]
                emit(dict(bias="call, in standard errors", model=name, scheme=scheme, points=N, steps=n, strikes=[100.0, 120.0],
                          anchors=[anchors[100.0], anchors[120.0]], prices=[float(prices[0, 0]), float(prices[1, 0])],
                          std_errors=[float(errors[0, 0]), float(errors[1, 0])], bias_in_std_errors=bias))
                if scheme == "euler" and euler_inside is None and max(abs(b) for b in bias) <= 3.0:
                    euler_inside = n
        emit(dict(euler_steps_inside_3_sigma=euler_inside if euler_inside is not None else "none at <= 1024 steps", model=name, points=N))

    # 3. the device's paths against the restatement (the ties of tests/test_gpu_heston_qe.py) and the share of exponential steps
    from tools.probe import binding as probe

    for N, n in ((1000, 7), (4133, 16), (200, 33)):
        for name, model in qe.MODELS.items():
            p = pricer(model)
            rows = {}
            for seed in (0, 5):
                spot, var, quadratic, psi = qe.paths(S, model, R, Q, T, n, *qe.sobol_draws(n, N, seed))
                keep = ~np.any(np.abs(psi - qe.PSI_C) < 1e-9, axis=1)
                got_spot, got_var = p.simulate_paths(S, T, R, Q, N, n, seed, method="qmc", path_construction="sequential", scheme="qe")
                rows[f"sobol_seed{seed}"] = dict(spot_rel=worst(got_spot[keep], spot[keep], 1e-300), var_abs=float(np.max(np.abs(got_var[keep] - var[keep]))),
                                                 set_aside=int((~keep).sum()), exponential_share=float(1.0 - quadratic.mean()))
            if n <= 16:
                words = philox_oracle.philox_words(3, 0, N, 0, n, qe.STREAM_HESTON_QE)
                spot, var, quadratic, psi = qe.paths(S, model, R, Q, T, n, *qe.philox_draws(words, probe.box_muller_probe))
                keep = ~np.any(np.abs(psi - qe.PSI_C) < 1e-9, axis=1)
                got_spot, got_var = p.simulate_paths(S, T, R, Q, N, n, 3, scheme="qe")
                rows["philox_seed3"] = dict(spot_rel=worst(got_spot[keep], spot[keep], 1e-300), var_abs=float(np.max(np.abs(got_var[keep] - var[keep]))),
                                            set_aside=int((~keep).sum()), exponential_share=float(1.0 - quadratic.mean()))
            emit(dict(tie="device paths against tests/heston_qe_reference.py", model=name, points=N, steps=n, **rows))

    # 4. the scatter of the at-the-money call over 16 scrambles against 16 Philox seeds at 2^14 x 16
    N, n = 1 << 14, 16
    for name in BIAS_MODELS:
        p = pricer(qe.MODELS[name])
        pseudo = np.array([p.price_monte_carlo(S, 100.0, T, R, Q, "call", N, n, 1000 + s, scheme="qe") for s in range(16)])
        sobol = np.array([p.price_monte_carlo(S, 100.0, T, R, Q, "call", N, n, s, method="qmc", path_construction="sequential", scheme="qe")
                          for s in range(16)])
        emit(dict(scatter="atm_call, scheme qe", model=name, points=N, steps=n, seeds=16, anchor=qe.heston_call(S, 100.0, T, R, Q, qe.MODELS[name]),
                  mean_philox=float(pseudo.mean()), sd_philox=float(pseudo.std(ddof=1)), mean_sequential=float(sobol.mean()),
                  sd_sequential=float(sobol.std(ddof=1)), philox_over_sequential=float(pseudo.std(ddof=1) / sobol.std(ddof=1))))
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
