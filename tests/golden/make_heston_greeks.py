#!/usr/bin/env python3
"""Generate tests/golden/heston_greeks.json by RUNNING the reference.

Run only where the reference checkout that make_heston_surface.py names (its REF) is mounted:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_heston_greeks.py

The reference has no Greeks of its Heston Monte Carlo price: its HestonAdapter bumps the semi-analytic price_european.  What it does
have is compute_greeks_unified over ANY object with a .price(S, K, T, r, sigma, option_type, q), so this script runs it over a
five-line adapter that calls the reference's HestonPricer.price_monte_carlo(..., seed=s) with v0 = sigma^2 -- HestonAdapter's own
convention -- once per NumPy seed s: every bump of one Greeks computation sees the same stream, as the device's fused launch does.
Cases: at the money, n_steps = 64, both models, call and put, sigma = sqrt(v0).  Per case and Greek the fixture holds the mean over
the seeds and the standard error of that mean (std(ddof=1) / sqrt(seeds)); the test computes the same statistics on the device and
compares at five combined standard errors.  The scheme and n_steps are the same on both sides, so Euler's bias cancels.  The fixture
holds numbers only.  The reference is imported through the stub packages of make_heston_surface.py.
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_heston_surface as surface                                           # noqa: E402  (its REF, MODELS and stub loader)

OUT = os.path.join(HERE, "heston_greeks.json")
S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.02
N, STEPS, SEEDS = 50_000, 64, tuple(range(7001, 7017))                          # minutes of NumPy for 16 x 4 x 14 prices
GREEKS = ("price", "delta", "gamma", "vega", "theta", "rho", "vanna", "charm", "vomma")


def load_reference():
    HestonPricer, _iv = surface.load_reference()
    for name, rel in (("src.greeks", "src/greeks"), ("src.exceptions", "src/exceptions")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(surface.REF, rel)]
        sys.modules[name] = pkg
    from src.greeks.unified_greeks import compute_greeks_unified

    return HestonPricer, compute_greeks_unified


class MonteCarloAdapter:
    def __init__(self, model_cls, model, seed):
        self.model_cls, self.model, self.seed = model_cls, model, seed

    def price(self, S_, K_, T_, r_, sigma, option_type, q=0.0, **kwargs):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)                      # Feller
            pricer = self.model_cls(*self.model[:4], sigma**2)
        return float(pricer.price_monte_carlo(S_, K_, T_, r_, q, option_type, N, STEPS, seed=self.seed))


def main():
    import numpy as np

    HestonPricer, compute_greeks_unified = load_reference()
    doc = {"generator": "tests/golden/make_heston_greeks.py", "numpy": np.__version__,
           "inputs": dict(S=S, K=K, T=T, r=R, q=Q, n_paths=N, n_steps=STEPS, numpy_seeds=list(SEEDS)),
           "models": {k: list(v) for k, v in surface.MODELS.items()}, "greeks": []}
    for model_name, model in surface.MODELS.items():
        sigma = float(np.sqrt(model[4]))
        for option_type in ("call", "put"):
            runs = []
            for seed in SEEDS:
                g = compute_greeks_unified(MonteCarloAdapter(HestonPricer, model, seed), S, K, T, R, sigma, option_type, Q)
                runs.append([float(g[name]) for name in GREEKS])
            runs = np.asarray(runs)
            row = dict(model=model_name, option_type=option_type, sigma=sigma)
            for j, name in enumerate(GREEKS):
                row[name] = dict(mean=float(np.mean(runs[:, j])), std_error=float(np.std(runs[:, j], ddof=1) / np.sqrt(len(SEEDS))))
            doc["greeks"].append(row)
            print(model_name, option_type, {name: (row[name]["mean"], row[name]["std_error"]) for name in GREEKS}, flush=True)
    assert len(doc["greeks"]) == 4
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
