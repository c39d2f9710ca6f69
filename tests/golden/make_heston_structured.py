#!/usr/bin/env python3
"""Generate tests/golden/heston_structured.json: the autocallable and the cliquet under Heston on the product's own grid of 12 steps.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_heston_structured.py

Both payoffs are the reference's, in oracle/numpy_reference.py's restatements (autocallable_from_paths, cliquet_from_paths), applied to a
spot matrix of N = 2^22 paths:

  scheme "qe"     tests/heston_qe_reference.py's paths under FELLER_VIOLATED and STEEP, draws from numpy.random.default_rng(42) in
                  chunks of 2^18 paths (per chunk: U_v, Z_v, Z_s, each (chunk, 12)).  Needs nothing but this repository.
  scheme "euler"  the reference's HestonPricer.simulate_paths(S, T, r, q, N, 12, 42) under heston_path_oracle.USUAL.  Needs the reference
                  checkout (OLMC_REFERENCE, as make_heston_path_payoffs.py; imported by the stub-package recipe of SURVEY 8(c)).

Each entry stores the price and its standard error: the autocallable's payoffs carry their own discount (price = mean), the cliquet's
are discounted once (price = exp(-r T) mean).  The QE entries come first, so that the first entry can be reproduced anywhere
(tests/test_heston_structured_cpu.py runs qe_entries at a reduced N).  The fixture holds numbers only.
"""
import json
import math
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("OLMC_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "heston_structured.json")

S, T, R, Q = 100.0, 1.0, 0.05, 0.01
N, STEPS, SEED, CHUNK = 1 << 22, 12, 42, 1 << 18
AUTOCALLABLE = dict(autocall_barrier=1.0, coupon_barrier=0.9, ki_barrier=0.8, coupon_rate=0.10, observation_freq=3)      # quarterly
CLIQUET = dict(local_cap=0.05, local_floor=-0.05, global_cap=0.30, global_floor=0.0, n_periods=12)                       # monthly
QE_MODELS = ("feller_violated", "steep")


def payoffs(spot):
    """{payoff: per-path values whose plain mean times `discount` is the price}, discount per payoff."""
    sys.path.insert(0, ROOT)
    from oracle import numpy_reference as orc

    a = AUTOCALLABLE
    auto = orc.autocallable_from_paths(spot, S, T, R, a["observation_freq"], a["autocall_barrier"], a["coupon_barrier"], a["coupon_rate"],
                                       a["ki_barrier"], return_payoffs=True)[1]
    c = CLIQUET
    cliq = orc.cliquet_from_paths(spot, S, T, R, c["n_periods"], c["local_cap"], c["local_floor"], c["global_cap"], c["global_floor"],
                                  return_payoffs=True)[1]
    return {"cliquet": (cliq, math.exp(-R * T)), "autocallable": (auto, 1.0)}


class Moments:
    def __init__(self):
        self.n, self.sum, self.sumsq = 0, 0.0, 0.0

    def add(self, x):
        import numpy as np

        self.n += x.size
        self.sum += float(np.sum(x))
        self.sumsq += float(np.sum(x * x))

    def entry(self, discount, **labels):
        mean = self.sum / self.n
        var = max(self.sumsq / self.n - mean * mean, 0.0)
        return dict(**labels, price=discount * mean, std_error=discount * math.sqrt(var / self.n))


def qe_entries(model_name, n_paths=N, chunk=CHUNK):
    """[cliquet, autocallable] under the QE restatement: default_rng(SEED), chunks of `chunk` paths."""
    import numpy as np

    sys.path.insert(0, ROOT)
    from tests import heston_qe_reference as qe

    model = qe.MODELS[model_name]
    rng = np.random.default_rng(SEED)
    moments = {"cliquet": Moments(), "autocallable": Moments()}
    discount = {}
    for first in range(0, n_paths, chunk):
        m = min(chunk, n_paths - first)
        u_v, z_v, z_s = rng.random((m, STEPS)), rng.standard_normal((m, STEPS)), rng.standard_normal((m, STEPS))
        spot = qe.paths(S, model, R, Q, T, STEPS, u_v, z_v, z_s)[0]
        for name, (x, d) in payoffs(spot).items():
            moments[name].add(x)
            discount[name] = d
    return [moments[name].entry(discount[name], scheme="qe", model=model_name, payoff=name) for name in ("cliquet", "autocallable")]


def load_reference():
    for name, rel in (("src", "src"), ("src.pricing_models", "src/pricing_models")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    sys.path.insert(0, REF)
    from src.pricing_models.heston import HestonPricer

    return HestonPricer


def euler_entries(n_paths=N):
    """[cliquet, autocallable] on the reference's own Euler paths under heston_path_oracle.USUAL."""
    sys.path.insert(0, ROOT)
    from tests import heston_path_oracle as hpo

    HestonPricer = load_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        spot = HestonPricer(*hpo.USUAL).simulate_paths(S, T, R, Q, n_paths, STEPS, SEED)[0]
    out = []
    for name, (x, d) in payoffs(spot).items():
        mo = Moments()
        mo.add(x)
        out.append(mo.entry(d, scheme="euler", model="usual", payoff=name))
    return out


def main():
    import numpy as np

    sys.path.insert(0, ROOT)
    from tests import heston_path_oracle as hpo
    from tests import heston_qe_reference as qe

    doc = {"generator": "tests/golden/make_heston_structured.py", "numpy": np.__version__,
           "inputs": dict(S=S, T=T, r=R, q=Q, n_paths=N, n_steps=STEPS, numpy_seed=SEED, chunk=CHUNK),
           "autocallable": AUTOCALLABLE, "cliquet": CLIQUET,
           "models": {**{k: list(qe.MODELS[k]) for k in QE_MODELS}, "usual": list(hpo.USUAL)}, "prices": []}
    for model_name in QE_MODELS:
        doc["prices"] += qe_entries(model_name)
    doc["prices"] += euler_entries()
    assert len(doc["prices"]) == 6
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['prices'])} prices")
    for e in doc["prices"]:
        print(e)


if __name__ == "__main__":
    main()
