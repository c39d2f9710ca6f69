#!/usr/bin/env python3
"""Generate tests/golden/local_vol.json by RUNNING the reference's src/pricing_models/local_vol.py.

    OPTIONSLAB_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_local_vol.py

For the reference's own sample surface, create_sample_iv_surface() (20 strikes x 5 expiries, q = 0), and for one 7 x 3 surface with
q != 0 the fixture records
  - DupireLocalVol.dupire_formula's matrix (floor cells at sqrt(0.001) and fallback cells included, flagged by the script), and
  - the calibrated surface, LocalVolSurface.__call__, at 39 points (K, T): 13 strikes x 3 times, of which 4 strikes lie below the
    first node, 4 above the last, and one time before the first expiry and one after the last -- the reference's spline holds the
    surface flat outside its nodes, and these values pin that.
A 7 x 3 surface has too few expiries for the reference's bicubic spline (RectBivariateSpline needs four): its `calibrate` raises, and
the fixture records the exception's type instead of surface values.  So that the spline is tied with q != 0 too, a third case adds one
expiry to that surface (7 x 4) and records both.  The fixture holds numbers and names only.  The reference is
imported by the stub-package recipe, as make_heston_surface.py does.
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "local_vol.json")

SMALL = dict(spot=50.0, r=0.03, q=0.02, strikes=[35.0, 40.0, 45.0, 50.0, 55.0, 60.0, 65.0], expiries=[0.25, 0.5, 1.0])
SMALL4 = dict(SMALL, expiries=[0.25, 0.5, 0.75, 1.0])          # one expiry more: the smallest surface the spline accepts, so q != 0 reaches it


def load_reference(ref):
    for name, rel in (("src", "src"), ("src.pricing_models", "src/pricing_models")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(ref, rel)]
        sys.modules[name] = pkg
    sys.path.insert(0, ref)
    from src.pricing_models.local_vol import DupireLocalVol, create_sample_iv_surface

    return DupireLocalVol, create_sample_iv_surface


def small_iv(np, small=SMALL):
    k, t = np.asarray(small["strikes"]), np.asarray(small["expiries"])
    m = np.log(k / small["spot"])[None, :]
    return 0.22 + 0.03 * np.sqrt(t)[:, None] + (0.12 * m**2 - 0.08 * m) * np.sqrt(0.25 / t)[:, None]


def probe_points(np, strikes, expiries):
    lo, hi = float(strikes[0]), float(strikes[-1])
    ks = [0.5 * lo, 0.8 * lo, 0.95 * lo, lo - 1e-3] + list(np.linspace(lo, hi, 5) * [1.0, 1.013, 0.997, 1.021, 1.0]) + [hi + 1e-3, 1.05 * hi, 1.3 * hi, 2.0 * hi]
    ts = [0.5 * float(expiries[0]), 0.37 * float(expiries[0]) + 0.63 * float(expiries[-1]), 1.5 * float(expiries[-1])]
    return [(float(k), float(t)) for t in ts for k in ks]


def record(np, DupireLocalVol, name, strikes, expiries, iv, spot, r, q):
    model = DupireLocalVol(r=r, q=q)
    lv = model.dupire_formula(strikes, expiries, iv, spot)
    floor = float(np.sqrt(0.001))
    inner = lv[1:, 1:-1]
    doc = dict(name=name, spot=spot, r=r, q=q, strikes=[float(k) for k in strikes], expiries=[float(t) for t in expiries],
               iv=[[float(v) for v in row] for row in iv], local_vol=[[float(v) for v in row] for row in lv],
               floor_cells=[[int(i), int(j)] for i, j in zip(*np.nonzero(lv == floor))],          # the boundary columns copy their neighbours
               fallback_cells=[[int(i) + 1, int(j) + 1] for i, j in zip(*np.nonzero(inner == iv[1:, 1:-1]))])
    try:
        surface = DupireLocalVol(r=r, q=q).calibrate(strikes, expiries, iv, spot)
    except Exception as e:                                   # too few nodes for the bicubic spline
        doc["calibrate_raises"] = type(e).__name__
        return doc
    doc["surface"] = [dict(K=k, T=t, value=float(surface(k, t))) for k, t in probe_points(np, strikes, expiries)]
    return doc


def main():
    import numpy as np
    import scipy

    ref = os.environ.get("OPTIONSLAB_REFERENCE")
    if not ref:
        sys.exit("set OPTIONSLAB_REFERENCE to a checkout of the reference")
    DupireLocalVol, create_sample_iv_surface = load_reference(ref)
    strikes, expiries, iv = create_sample_iv_surface()
    cases = [record(np, DupireLocalVol, "sample", strikes, expiries, iv, 100.0, 0.05, 0.0),
             record(np, DupireLocalVol, "small_q", np.asarray(SMALL["strikes"]), np.asarray(SMALL["expiries"]), small_iv(np), SMALL["spot"],
                    SMALL["r"], SMALL["q"]),
             record(np, DupireLocalVol, "small_q_four_expiries", np.asarray(SMALL4["strikes"]), np.asarray(SMALL4["expiries"]), small_iv(np, SMALL4),
                    SMALL4["spot"], SMALL4["r"], SMALL4["q"])]
    doc = {"generator": "tests/golden/make_local_vol.py", "numpy": np.__version__, "scipy": scipy.__version__, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for c in cases:
        print(f"{c['name']}: {len(c['floor_cells'])} floor cells, {len(c['fallback_cells'])} fallback cells, "
              f"{len(c.get('surface', []))} surface points, calibrate raises {c.get('calibrate_raises')}")


if __name__ == "__main__":
    main()
