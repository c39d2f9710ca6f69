#!/usr/bin/env python3
"""Generate tests/golden/sabr.json by RUNNING the reference's src/pricing_models/sabr.py.

    OPTIONSLAB_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sabr.py

The fixture records
  - SABRModel.implied_vol and SABRModel.price (call and put, r = 0.03) on a grid: beta in {0, 0.5, 0.7, 1}, alpha = 0.25 F^(1 - beta),
    three (rho, nu) pairs (a mild one, a steep one, nu = 0), strikes on and off the money -- among them K = F, K = F + 5e-11 (inside the
    reference's at-the-money window |K - F| < 1e-10) and K = F (1 + 1e-9) (outside it, with |z| < 1e-7: the z / x(z) = 1 branch) --,
    and T in {0, 0.25, 1, 5}; each row is flagged with the branch the reference takes;
  - four calibrate_sabr results on noise-free 13-strike smiles (K from 70 % to 130 % of F, T = 1) the reference's own model draws:
    alpha 0.25 beta 1 rho -0.4 nu 0.5; alpha 0.9 beta 0.7 rho 0.2 nu 0.6; a rates-like F = 0.03, beta 0.5, alpha 0.035; and alpha 2.5,
    beta 0.5, which the reference drives onto its alpha <= 2.0 bound (the quirk is pinned as it is).
The fixture holds numbers and names only.  The reference is imported by the stub-package recipe, as make_local_vol.py does.
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sabr.json")

F, R = 100.0, 0.03
BETAS = (0.0, 0.5, 0.7, 1.0)
RHO_NU = ((-0.3, 0.4), (-0.7, 0.8), (0.2, 0.0))
STRIKES = (60.0, 80.0, 95.0, 100.0, 100.0 + 5e-11, 100.0 * (1 + 1e-9), 105.0, 120.0, 150.0)
TIMES = (0.0, 0.25, 1.0, 5.0)

# name, F, truth (alpha, beta, rho, nu)
CALIBRATIONS = (("lognormal", 100.0, (0.25, 1.0, -0.4, 0.5)), ("general", 100.0, (0.9, 0.7, 0.2, 0.6)),
                ("rates", 0.03, (0.035, 0.5, -0.2, 0.45)), ("alpha-bound", 100.0, (2.5, 0.5, -0.3, 0.4)))


def load_reference(ref):
    for name, rel in (("src", "src"), ("src.pricing_models", "src/pricing_models")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(ref, rel)]
        sys.modules[name] = pkg
    sys.path.insert(0, ref)
    from src.pricing_models.sabr import SABRModel, calibrate_sabr

    return SABRModel, calibrate_sabr


def branch(np, model, K, T):
    if T <= 0:
        return "expired"
    if abs(K - F) < 1e-10:
        return "atm"
    z = (model.nu / model.alpha) * (F * K) ** ((1 - model.beta) / 2) * np.log(F / K)
    return "small-z" if abs(z) < 1e-7 else "general"


def main():
    import numpy as np
    import scipy

    ref = os.environ.get("OPTIONSLAB_REFERENCE")
    if not ref:
        sys.exit("set OPTIONSLAB_REFERENCE to a checkout of the reference")
    SABRModel, calibrate_sabr = load_reference(ref)
    warnings.simplefilter("ignore")                          # nu = 0: the reference evaluates 0 / 0 before it takes the small-z branch
    grid = []
    for beta in BETAS:
        for rho, nu in RHO_NU:
            model = SABRModel(0.25 * F ** (1 - beta), beta, rho, nu)
            for K in STRIKES:
                for T in TIMES:
                    grid.append(dict(alpha=model.alpha, beta=beta, rho=rho, nu=nu, F=F, K=K, T=T, r=R, branch=branch(np, model, K, T),
                                     implied_vol=float(model.implied_vol(F, K, T)), call=float(model.price(F, K, T, R, "call")),
                                     put=float(model.price(F, K, T, R, "put"))))
    fits = []
    for name, forward, truth in CALIBRATIONS:
        strikes = np.linspace(0.7 * forward, 1.3 * forward, 13)
        vols = SABRModel(*truth).smile(forward, 1.0, strikes)
        fit = calibrate_sabr(forward, 1.0, strikes, vols, beta=truth[1])
        fits.append(dict(name=name, F=forward, T=1.0, truth=list(truth), strikes=[float(k) for k in strikes], market_vols=[float(v) for v in vols],
                         fitted=[float(fit.alpha), float(fit.beta), float(fit.rho), float(fit.nu)]))
    doc = {"generator": "tests/golden/make_sabr.py", "numpy": np.__version__, "scipy": scipy.__version__, "grid": grid, "calibrations": fits}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    count = {}
    for row in grid:
        count[row["branch"]] = count.get(row["branch"], 0) + 1
    print(f"{len(grid)} grid rows by branch {count}")
    for c in fits:
        print(c["name"], "truth", c["truth"], "fitted", c["fitted"])


if __name__ == "__main__":
    main()
