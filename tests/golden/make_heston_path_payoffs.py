#!/usr/bin/env python3
"""Generate tests/golden/heston_path_payoffs.json by RUNNING the reference.

Run only in the build container, where /root/reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_heston_path_payoffs.py

The reference has no Asian, barrier or lookback option under Heston as one call; it has the three option classes, whose price()
reads a spot matrix from _generate_paths, and HestonPricer.simulate_paths, which makes one.  This script joins them as a user of the
reference would: _generate_paths of AsianOption, BarrierOption and LookbackOption is patched to return
HestonPricer.simulate_paths(...)[0] for a fixed NumPy seed, and each class's own price() runs on it.  Next to each price it records
exp(-r T) std / sqrt(N) of the same payoffs (oracle/numpy_reference.py's restatements, checked here to give the reference's price to
1e-12).  The fixture holds numbers only.  The reference is imported by the stub-package recipe of SURVEY §8(c), as make_golden.py does.
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "heston_path_payoffs.json")

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
UP, DOWN = 120.0, 85.0
N, STEPS, SEED = 100_000, 64, 20240611
MODELS = {"usual": (2.0, 0.04, 0.3, -0.7, 0.04), "feller_violating": (3.0, 0.02, 0.8, 0.3, 0.05)}     # kappa theta sigma_v rho v0


def load_reference():
    for name, rel in (("src", "src"), ("src.pricing_models", "src/pricing_models")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    sys.path.insert(0, REF)
    from src.pricing_models.exotic_options import AsianOption, BarrierOption, LookbackOption
    from src.pricing_models.heston import HestonPricer

    return AsianOption, BarrierOption, LookbackOption, HestonPricer


def main():
    import numpy as np

    sys.path.insert(0, ROOT)
    from oracle import numpy_reference as orc

    AsianOption, BarrierOption, LookbackOption, HestonPricer = load_reference()
    doc = {"generator": "tests/golden/make_heston_path_payoffs.py", "numpy": np.__version__,
           "inputs": dict(S=S, K=K, T=T, r=R, q=Q, up_barrier=UP, down_barrier=DOWN, n_paths=N, n_steps=STEPS, numpy_seed=SEED),
           "models": {k: list(v) for k, v in MODELS.items()}, "prices": []}
    for model_name, model in MODELS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)                      # Feller
            spot = HestonPricer(*model).simulate_paths(S, T, R, Q, N, STEPS, SEED)[0]
        for cls in (AsianOption, BarrierOption, LookbackOption):
            cls._generate_paths = lambda self, n_paths, n_steps: spot

        def record(payoff, option_type, price, x):
            want = float(np.exp(-R * T) * np.mean(x))
            assert abs(float(price) - want) <= 1e-12 * max(1.0, abs(want)), (payoff, option_type, price, want)
            doc["prices"].append(dict(model=model_name, payoff=payoff, option_type=option_type, price=float(price),
                                      std_error=float(np.exp(-R * T) * np.std(x) / np.sqrt(N))))

        for option_type in ("call", "put"):
            for avg_type in ("arithmetic", "geometric"):
                price = AsianOption(S, K, T, R, 0.2, Q).price(N, STEPS, avg_type, option_type)
                record(f"asian-{avg_type}", option_type, price, orc.asian_from_paths(spot, K, T, R, avg_type, option_type, True)[1])
            for kind in ("up-and-out", "up-and-in", "down-and-out", "down-and-in"):
                level = UP if kind.startswith("up") else DOWN
                price = BarrierOption(S, K, T, R, 0.2, Q, barrier=level).price(N, STEPS, kind, option_type)
                record(f"barrier-{kind}", option_type, price, orc.barrier_from_paths(spot, K, T, R, level, kind, option_type, True)[1])
            for kind in ("floating", "fixed"):
                price = LookbackOption(S, K, T, R, 0.2, Q).price(N, STEPS, kind, option_type)
                record(f"lookback-{kind}", option_type, price, orc.lookback_from_paths(spot, K, T, R, kind, option_type, True)[1])
    assert len(doc["prices"]) == 32
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['prices'])} prices")


if __name__ == "__main__":
    main()
