#!/usr/bin/env python3
"""Interleaved A/B of whole libolmc builds: one subprocess per (library, round), each timing the
European path kernel with HIP events (olmc_kernel_time).  --case takes one name or a comma-separated list (measured one after the other in the
same subprocess, which is ended after --timeout seconds); --out appends one JSON line per (case, library).  Usage (GPU box):
    python tools/ab_libs.py libA.so libB.so ... [--n 1000000] [--m 252] [--rounds 7] [--timeout 300] [--out FILE.jsonl] [--case european|heston_*|greeks8|greeks14|greeks8_lean|greeks14_lean|asian|asian_fast|asian_fast_anti|asian_anti|asian_geo|barrier|heston|merton|kou|autocall[_anti]|cliquet[_anti]|american|{barrier,lookback}_greeks{8,14}[_anti]|asian_greeks8|asian_greeks14[_rho]|qmc|qmc_cv|qmc_greeks8|qmc_greeks14|lv_{european,asian,asian_geo,lookback,barrier,surface}[_anti]|lvq_{...}_{seq,bridge}[_anti]|jd_surface_{merton,kou}[_anti]]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import json, sys
sys.path.insert(0, %r)
from optionslab_amd import _hip
N, M = int(sys.argv[1]), int(sys.argv[2])
_hip.lib(); _hip.profile_enable(True)
P = (100.0, 100.0, 1.0, 0.05, 0.2, 0.0)
CASES = {
    "european": lambda s: _hip.european(*P, True, N, M, s, True),
    "greeks8": lambda s: _hip.european_greeks_fd(*P, True, N, M, s, False)[1][0],
    "greeks14": lambda s: _hip.european_greeks_fd(*P, True, N, M, s, True)[1][0],
    # the call MonteCarloPricer.greeks() makes: no per-evaluation statistics asked for (prices-only kernel from round 3 on)
    "greeks8_lean": lambda s: type("R", (), dict(zip(("price", "sum"), (lambda v: (v[0], v[1]))(_hip.european_greeks_fd(*P, True, N, M, s, False, want_evals=False)[0]))))(),
    "greeks14_lean": lambda s: type("R", (), dict(zip(("price", "sum"), (lambda v: (v[0], v[8]))(_hip.european_greeks_fd(*P, True, N, M, s, True, want_evals=False)[0]))))(),
    "asian": lambda s: _hip.asian(*P, True, False, N, M, s, False),
    "asian_fast": lambda s: _hip.asian(*P, True, False, N, M, s, False, fast=True),
    "asian_fast_anti": lambda s: _hip.asian(*P, True, False, N, M, s, True, fast=True),
    "asian_anti": lambda s: _hip.asian(*P, True, False, N, M, s, True),
    "asian_geo": lambda s: _hip.asian(*P, True, True, N, M, s, False),
    "barrier": lambda s: _hip.barrier(*P, True, 120.0, 0, N, M, s, False),
    "merton": lambda s: _hip.jump_diffusion(*P, True, False, 0.5, -0.1, 0.2, 0.0, N, M, s),
    "kou": lambda s: _hip.jump_diffusion(*P, True, True, 1.0, 0.4, 10.0, 5.0, N, M, s),
    "autocall": lambda s: _hip.autocallable(100.0, 1.0, 0.05, 0.2, 0.0, 1.0, 0.8, 0.08, 0.6, 21, N, M, s),
    "autocall_anti": lambda s: _hip.autocallable(100.0, 1.0, 0.05, 0.2, 0.0, 1.0, 0.8, 0.08, 0.6, 21, N, M, s, True),
    "cliquet": lambda s: _hip.cliquet(100.0, 1.0, 0.05, 0.2, 0.0, 0.05, -0.05, 0.3, 0.0, 12, N, M, s),
    "cliquet_anti": lambda s: _hip.cliquet(100.0, 1.0, 0.05, 0.2, 0.0, 0.05, -0.05, 0.3, 0.0, 12, N, M, s, True),
    "heston": lambda s: _hip.heston(100.0, 100.0, 1.0, 0.05, 0.0, True, 2.0, 0.04, 0.3, -0.7, 0.04, N, M, s, False),
}
# round 4: the per-date launches of the American option, and the Sobol kernels (a table of `M` dimensions built once, seed 42)
CASES["asian_greeks8"] = lambda s: _hip.asian_greeks_fd(*P, True, N, M, s, False, False)[1][0]
CASES["asian_greeks14"] = lambda s: _hip.asian_greeks_fd(*P, True, N, M, s, False, True)[1][0]
CASES["asian_greeks14_rho"] = lambda s: _hip.asian_greeks_fd(*P, True, N, M, s, False, True)[1][6]       # the r + h evaluation
CASES["american"] = lambda s: _hip.american_lsm(*P, False, N, M, 3, s)
# round 5: the fused barrier / lookback Greeks (payoff 0 = up-and-out barrier at 120, 4 = floating lookback), 8 / 14 contracts, +- antithetic
for _name, _payoff, _level in (("barrier", 0, 120.0), ("lookback", 4, 0.0)):
    for _k, _second in ((8, False), (14, True)):
        for _anti in (False, True):
            CASES[f"{_name}_greeks{_k}" + ("_anti" if _anti else "")] = (lambda s, p=_payoff, l=_level, a=_anti, o=_second: _hip.extrema_greeks_fd(*P, True, p, l, N, M, s, a, o)[1][0])
if sys.argv[3].startswith("qmc"):
    import numpy as np
    from optionslab_amd.monte_carlo import sobol_tables
    SV, SH = sobol_tables(M, 42)
    CASES["qmc"] = lambda s: _hip.european_qmc(*P, True, N, SV, SH)
    CASES["qmc_cv"] = lambda s: (lambda m: type("R", (), dict(price=m.value, sum=m.sum_d))())(_hip.european_qmc_cv(*P, True, N, SV, SH))
    CASES["qmc_greeks8"] = lambda s: _hip.european_qmc_greeks_fd(*P, True, N, SV, SH, False)[1][0]
    CASES["qmc_greeks14"] = lambda s: _hip.european_qmc_greeks_fd(*P, True, N, SV, SH, True)[1][0]
# the Heston family: M steps (Sobol: 2 M dimensions, seed 42), the usual model for Euler and a Feller-violating one (both branches) for QE
HM, HQ = (2.0, 0.04, 0.3, -0.7, 0.04), (1.0, 0.09, 1.0, -0.3, 0.09)
HA, HC = (1.0, 0.9, 0.10, 0.8, 21), (0.05, -0.05, 0.30, 0.0, 12)
if "heston_" in sys.argv[3]:
    from optionslab_amd.monte_carlo import sobol_tables
    HSV, HSH = sobol_tables(2 * M, 42, N) if "qmc" in sys.argv[3] else (None, None)
    one = lambda cells: type("R", (), dict(price=cells[0].price, sum=cells[0].sum))()
    head = lambda mats: type("R", (), dict(price=float(mats[0][-1].mean()), sum=float(mats[1][-1].sum())))()
    for _a, _sa in ((False, ""), (True, "_anti")):
        CASES["heston" + _sa] = lambda s, a=_a: _hip.heston(100.0, 100.0, 1.0, 0.05, 0.0, True, *HM, N, M, s, a)
        CASES["heston_surface" + _sa] = lambda s, a=_a: one(_hip.heston_surface(100.0, 1.0, 0.05, 0.0, True, *HM, [100.0], [M], N, M, s, a))
        CASES["heston_qe_surface" + _sa] = lambda s, a=_a: one(_hip.heston_qe_surface(100.0, 1.0, 0.05, 0.0, True, *HQ, [100.0], [M], N, M, s, a))
        CASES["heston_qe_qmc_surface" + _sa] = lambda s, a=_a: one(_hip.heston_qe_qmc_surface(100.0, 1.0, 0.05, 0.0, True, *HQ, [100.0], [M], N, HSV, HSH, False, a))
        for _q, _sq, _m in ((False, "", HM), (True, "_qe", HQ)):
            CASES["heston_autocall" + _sq + _sa] = lambda s, a=_a, q=_q, m=_m: _hip.heston_autocallable(100.0, 1.0, 0.05, 0.0, *m, *HA, N, M, s, a, 0, q)
            CASES["heston_cliquet" + _sq + _sa] = lambda s, a=_a, q=_q, m=_m: _hip.heston_cliquet(100.0, 1.0, 0.05, 0.0, *m, *HC, N, M, s, a, 0, q)
            for _b, _sb in ((False, "_seq"), (True, "_bridge")):
                if _q and _b:
                    continue
                CASES["heston_qmc_autocall" + _sq + _sb + _sa] = lambda s, a=_a, q=_q, m=_m, b=_b: _hip.heston_autocallable_qmc(100.0, 1.0, 0.05, 0.0, *m, *HA, N, HSV, HSH, b, a, 0, q)
                CASES["heston_qmc_cliquet" + _sq + _sb + _sa] = lambda s, a=_a, q=_q, m=_m, b=_b: _hip.heston_cliquet_qmc(100.0, 1.0, 0.05, 0.0, *m, *HC, N, HSV, HSH, b, a, 0, q)
        for _b, _sb in ((False, "_seq"), (True, "_bridge")):
            CASES["heston_qmc" + _sb + _sa] = lambda s, a=_a, b=_b: _hip.heston_qmc(100.0, 100.0, 1.0, 0.05, 0.0, True, *HM, N, HSV, HSH, b, a)
            CASES["heston_qmc_surface" + _sb + _sa] = lambda s, a=_a, b=_b: one(_hip.heston_qmc_surface(100.0, 1.0, 0.05, 0.0, True, *HM, [100.0], [M], N, HSV, HSH, b, a))
            for _f, _payoff in (("asian", _hip.PATH_ASIAN_ARITHMETIC), ("asian_geo", _hip.PATH_ASIAN_GEOMETRIC), ("lookback", _hip.LOOKBACK_FLOATING)):
                if not _b:
                    CASES["heston_" + _f + _sa] = lambda s, a=_a, p=_payoff: _hip.heston_path_payoff(100.0, 100.0, 1.0, 0.05, 0.0, True, *HM, p, 0.0, N, M, s, a)
                CASES["heston_qmc_" + _f + _sb + _sa] = lambda s, a=_a, b=_b, p=_payoff: _hip.heston_qmc_path_payoff(100.0, 100.0, 1.0, 0.05, 0.0, True, *HM, p, 0.0, N, HSV, HSH, b, a)
    for _pm, _sp in ((False, ""), (True, "_pm")):          # the path matrices: N x (M + 1) doubles twice to the host per call
        CASES["heston_paths" + _sp] = lambda s, pm=_pm: head(_hip.heston_paths(100.0, 1.0, 0.05, 0.0, *HM, N, M, s, pm))
        CASES["heston_qe_paths" + _sp] = lambda s, pm=_pm: head(_hip.heston_qe_paths(100.0, 1.0, 0.05, 0.0, *HQ, N, M, s, pm))
# local volatility (lv_*, lvq_*: the 33 x 128 tables of tools/local_vol_timing.py and tools/local_vol_qmc_timing.py, Sobol seed 42) and the
# jump surfaces (jd_surface_*: the models and the 12 cells of tools/jump_payoff_timing.py); payoff codes 8, 6, 7, 4, 0
if any(p in sys.argv[3] for p in ("lv_", "lvq_", "jd_")):
    import numpy as np
    LQ, LUP = 0.01, 120.0
    def _smile(base, t_hi):
        x = np.linspace(-0.5, 0.45, 128)[None, :]
        return base - 0.25 * x + 0.4 * x * x + 0.05 * (np.arange(33)[:, None] / 32), -0.5, 0.45, t_hi
    LVT, LVQT = _smile(0.22, 1.0), _smile(0.22, 0.8)
    CELLS = ([90.0, 100.0, 110.0] * 4, [M // 4] * 3 + [M // 2] * 3 + [3 * M // 4] * 3 + [M] * 3)
    one = lambda cells: type("R", (), dict(price=cells[0].price, sum=cells[0].sum))()
    if "lvq_" in sys.argv[3]:
        from optionslab_amd.monte_carlo import sobol_tables
        LSV, LSH = sobol_tables(M, 42, N)
    for _a, _sa in ((False, ""), (True, "_anti")):
        CASES["lv_surface" + _sa] = lambda s, a=_a: one(_hip.lv_surface_prices(100.0, 1.0, 0.05, LQ, True, LVT, *CELLS, N, M, s, a))
        for _m, _model in (("merton", (False, 0.5, -0.1, 0.2, 0.0)), ("kou", (True, 1.0, 0.4, 10.0, 5.0))):
            CASES["jd_surface_" + _m + _sa] = lambda s, a=_a, m=_model: one(_hip.jd_surface_prices(100.0, 1.0, 0.05, 0.2, LQ, True, m, *CELLS, N, M, s, a))
        for _f, _code, _level in (("european", 8, 0.0), ("asian", 6, 0.0), ("asian_geo", 7, 0.0), ("lookback", 4, 0.0), ("barrier", 0, LUP)):
            CASES["lv_" + _f + _sa] = lambda s, a=_a, c=_code, l=_level: _hip.lv_price(100.0, 100.0, 1.0, 0.05, LQ, True, LVT, c, l, N, M, s, a)
            for _b, _sb in ((False, "_seq"), (True, "_bridge")):
                CASES["lvq_" + _f + _sb + _sa] = (lambda s, a=_a, c=_code, l=_level, b=_b:
                                                  _hip.lvq_price(100.0, 100.0, 1.0, 0.05, LQ, True, LVQT, c, l, N, LSV, LSH, b, a))
        for _b, _sb in ((False, "_seq"), (True, "_bridge")):
            CASES["lvq_surface" + _sb + _sa] = lambda s, a=_a, b=_b: one(_hip.lvq_surface_prices(100.0, 1.0, 0.05, LQ, True, LVQT, *CELLS, N, LSV, LSH, b, a))
import os, time
if os.environ.get("OLMC_AB_TUNE"):                      # "knob=value,knob=value" applied before anything runs
    for kv in os.environ["OLMC_AB_TUNE"].split(","):
        k, v = kv.split("=")
        _hip.tune(int(k), int(v))
for k, case in enumerate(sys.argv[3].split(",")):
    run = CASES[case]
    _hip.profile_enable(False)
    if k == 0:
        for i in range(400): run(1 + i)                      # clocks up (an idle device needs tens of ms of load)
    t0 = time.perf_counter()
    for i in range(100): st = run(42 + i)
    wall = (time.perf_counter() - t0) / 100
    _hip.profile_enable(True)
    _hip.profile_reset()
    for i in range(60): st = run(42 + i)
    n, ms = _hip.kernel_time()
    print(json.dumps({"case": case, "us": (ms / n * 1e3) if n else wall * 1e6, "wall_us": wall * 1e6, "price": st.price, "sum": st.sum}), flush=True)
""" % ROOT

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--m", type=int, default=252)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--case", default="european")
ap.add_argument("--out", default=None)
ap.add_argument("--timeout", type=float, default=300.0)
a = ap.parse_args()
cases = a.case.split(",")
# a library may carry a tuning suffix: "libolmc.so@7=-1" runs it with olmc_tune(7, -1) (e.g. split workgroups off)
res = {(c, l): [] for c in cases for l in a.libs}
wall = {(c, l): [] for c in cases for l in a.libs}
price = {}
for r in range(a.rounds):
    for l in a.libs:
        path, _, tune = l.partition("@")
        env = dict(os.environ, OLMC_LIBRARY=os.path.abspath(path))
        if tune:
            env["OLMC_AB_TUNE"] = tune
        out = subprocess.run([sys.executable, "-c", CHILD, str(a.n), str(a.m), a.case], env=env, capture_output=True, text=True, timeout=a.timeout)
        if out.returncode != 0:
            raise SystemExit(f"{l}: child failed (rc {out.returncode}): {out.stderr[-600:]}")
        for d in map(json.loads, out.stdout.strip().splitlines()[-len(cases):]):
            res[d["case"], l].append(d["us"])
            wall[d["case"], l].append(d["wall_us"])
            price[d["case"], l] = (d["price"], d["sum"])
for c, l in res:
    v, w = res[c, l], wall[c, l]
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(dict(case=c, lib=l, n=a.n, m=a.m, us=v, us_median=statistics.median(v), us_min=min(v), us_max=max(v),
                                    wall_us_median=statistics.median(w), price=price[c, l][0], sum=price[c, l][1])) + "\n")
    print(f"{c + ' ' if len(cases) > 1 else ''}{os.path.basename(l):34s} kernel median {statistics.median(v):8.2f} us  min {min(v):8.2f}  max {max(v):8.2f} | blocking call median "
          f"{statistics.median(w):8.2f} us | price {price[c, l][0]:.12f} sum {price[c, l][1]!r}", flush=True)
