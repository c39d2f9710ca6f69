#!/usr/bin/env python3
"""Generate tests/golden/heston_surface.json by RUNNING the reference.

Run only in the build container, where /root/reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_heston_surface.py

The reference prices one Heston contract per call; a strike x maturity surface is one HestonPricer.price_monte_carlo per cell.  Its
draws are per step, so for one NumPy seed and one step size the paths of a shorter maturity are a prefix of the longer one's: cell
(K, m) of the grid T m / n is the European payoff at column m of ONE simulate_paths(S, T, r, q, N, n, seed) matrix.  This script
records, per cell, the reference's price_monte_carlo(S, K, T m / n, r, q, type, N, m, seed) and exp(-r T_j) std(x) / sqrt(N) of the
payoffs x of that column, and asserts that the column's price agrees with price_monte_carlo's to 1e-12 (they agree exactly).  A second
section holds the reference's implied_volatility of every call price, with the `tolerance` its solver ran with.  The fixture holds
numbers only.  The reference is imported by the stub-package recipe of SURVEY §8(c), as make_golden.py does.
"""
import inspect
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "heston_surface.json")

S, T, R, Q = 100.0, 1.0, 0.05, 0.01
N, STEPS, SEED = 100_000, 64, 20240611
STRIKES, CELL_STEPS = (80.0, 100.0, 120.0), (16, 32, 64)
MODELS = {"usual": (2.0, 0.04, 0.3, -0.7, 0.04), "feller_violating": (3.0, 0.02, 0.8, 0.3, 0.05)}     # kappa theta sigma_v rho v0


def load_reference():
    for name, rel in (("src", "src"), ("src.pricing_models", "src/pricing_models")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    sys.path.insert(0, REF)
    from src.pricing_models.heston import HestonPricer
    from src.pricing_models.iv_solver import implied_volatility

    return HestonPricer, implied_volatility


def main():
    import numpy as np

    HestonPricer, implied_volatility = load_reference()
    tolerance = inspect.signature(implied_volatility).parameters["tolerance"].default
    doc = {"generator": "tests/golden/make_heston_surface.py", "numpy": np.__version__,
           "inputs": dict(S=S, T=T, r=R, q=Q, n_paths=N, n_steps=STEPS, numpy_seed=SEED, strikes=list(STRIKES), steps=list(CELL_STEPS)),
           "models": {k: list(v) for k, v in MODELS.items()}, "prices": [], "implied_vols": {"tolerance": tolerance, "rows": []}}
    worst = 0.0
    for model_name, model in MODELS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)                      # Feller
            pricer = HestonPricer(*model)
        spot = pricer.simulate_paths(S, T, R, Q, N, STEPS, SEED)[0]
        for option_type in ("call", "put"):
            sign = 1.0 if option_type == "call" else -1.0
            for m in CELL_STEPS:
                t_m = T * m / STEPS
                for strike in STRIKES:
                    price = float(pricer.price_monte_carlo(S, strike, t_m, R, Q, option_type, N, m, SEED))
                    x = np.maximum(sign * (spot[:, m] - strike), 0)
                    want = float(np.exp(-R * t_m) * np.mean(x))
                    worst = max(worst, abs(price - want) / max(1.0, abs(want)))
                    assert abs(price - want) <= 1e-12 * max(1.0, abs(want)), (model_name, option_type, m, strike, price, want)
                    doc["prices"].append(dict(model=model_name, option_type=option_type, strike=strike, step=m, maturity=t_m, price=price,
                                              std_error=float(np.exp(-R * t_m) * np.std(x) / np.sqrt(N))))
                    if option_type == "call":
                        doc["implied_vols"]["rows"].append(dict(model=model_name, strike=strike, maturity=t_m, price=price,
                                                                implied_vol=float(implied_volatility(price, S, strike, t_m, R, "call", Q))))
    assert len(doc["prices"]) == 36 and len(doc["implied_vols"]["rows"]) == 18
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['prices'])} prices, worst relative difference of the two routes {worst:.3g}")


if __name__ == "__main__":
    main()
