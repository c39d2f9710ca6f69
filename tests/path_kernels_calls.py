"""The calls of tests/golden/path_kernels_parent_bits.json, for its generator (tests/golden/make_path_kernels_parent_bits.py) and for
tests/test_gpu_path_kernels_parent_bits.py.  A helper, not a test module.

Every kernel that has the nine-payoff tail or shares the surface prologue, the wave-uniform Philox path loop, the local-volatility step
walk or a host runner with another one is called at the two smallest shapes at which those pieces can go wrong:
    257 paths x 13 steps    two workgroups; the last wave has ONE live lane (the `live` masking of the surface loops); 13 steps end in a
                            partial Philox block of four normals (local volatility, GBM) and of two (Heston, jumps);
    4133 paths x 5 steps    under tune(TUNE_GRID_CAP, 1): one workgroup strided over 17 trips, the last one partial.
Nothing here is an oracle: the fixture holds the words these calls gave on the commit before the pieces were shared.
"""
import hashlib

import numpy as np

from optionslab_amd import _hip
from tests import call_catalogue as cc
from tests import local_vol_oracle as lvo

S, K, T, R, Q, SIGMA = 100.0, 100.0, 1.0, 0.05, 0.01, 0.2
UP, DOWN = 112.0, 90.0
SEED = (0x9E3779B9 << 32) | 20240229
SHAPES = {"257x13": (257, 13, 0), "4133x5-cap1": (4133, 5, 1)}          # name: (paths, steps, TUNE_GRID_CAP)
TABLE = "33x128"                                                         # the fixture's name for the table: tests/test_gpu_local_vol.py's
TABLE_ARGS = lvo.smile_table(33, 128, -0.5, 0.45, 0.8).args
JUMPS = {"merton": (False, 0.5, -0.1, 0.2, 0.0), "kou": (True, 1.0, 0.4, 10.0, 5.0)}
PAYOFFS = tuple((code, UP if code < 2 else DOWN if code < 4 else 0.0) for code in range(9))     # 0 .. 3 barriers, 4 .. 7, 8 European
GROUPS = ("lv-price", "jd-price", "lvq-price", "surfaces", "matrices", "heston")


def cell_sets(n):
    return {"3cells": ([95.0, 105.0, 100.0], [n, 4, 5]), "1cell": ([100.0], [1])}


def scenarios():
    """Three scenarios on two recursions (the third has another maturity)."""
    return cc._scenario_set()[:3]


def calls(group, N, n):
    """{label: zero-argument callable} of one group at N paths (points) x n steps."""
    h, table = _hip, TABLE_ARGS
    one, two = (lambda: cc.tables(n, cc.SEED_A)), (lambda: cc.tables(2 * n, cc.SEED_A))      # a dimension per step / two per step
    sides = (("seq", False), ("bridge", True))
    out = {}
    if group == "lv-price":
        for code, level in PAYOFFS:
            for a in (0, 1):
                out[f"ollv_price-{code}-anti{a}"] = lambda code=code, level=level, a=a: h.lv_price(S, K, T, R, Q, True, table, code, level, N, n, SEED, bool(a))
    elif group == "jd-price":
        for name, model in JUMPS.items():
            for code, level in PAYOFFS:
                for a in (0, 1):
                    out[f"oljd_price-{name}-{code}-anti{a}"] = (lambda model=model, code=code, level=level, a=a:
                                                               h.jd_price(S, K, T, R, SIGMA, Q, True, model, code, level, N, n, SEED, bool(a)))
    elif group == "lvq-price":
        for code, level in PAYOFFS:
            for side, bridge in sides:
                for a in (0, 1):
                    out[f"olvq_price-{code}-{side}-anti{a}"] = (lambda code=code, level=level, bridge=bridge, a=a:
                                                               h.lvq_price(S, K, T, R, Q, True, table, code, level, N, *one(), bridge, bool(a)))
    elif group == "surfaces":
        for cells, (strikes, steps) in cell_sets(n).items():
            for a in ((0, 1) if cells == "3cells" else (0,)):
                tail = f"{cells}-anti{a}"
                out[f"ollv_surface_prices-{tail}"] = lambda strikes=strikes, steps=steps, a=a: h.lv_surface_prices(S, T, R, Q, True, table, strikes, steps, N, n, SEED, bool(a))
                for side, bridge in sides:
                    out[f"olvq_surface_prices-{side}-{tail}"] = (lambda strikes=strikes, steps=steps, a=a, bridge=bridge:
                                                                h.lvq_surface_prices(S, T, R, Q, True, table, strikes, steps, N, *one(), bridge, bool(a)))
                for name, model in JUMPS.items():
                    out[f"oljd_surface_prices-{name}-{tail}"] = (lambda strikes=strikes, steps=steps, a=a, model=model:
                                                                h.jd_surface_prices(S, T, R, SIGMA, Q, True, model, strikes, steps, N, n, SEED, bool(a)))
    elif group == "matrices":
        for layout, pm in (("step-major", False), ("path-major", True)):
            out[f"ollv_paths-{layout}"] = lambda pm=pm: h.lv_paths(S, T, R, Q, table, N, n, SEED, path_major=pm)
            out[f"olmc_gbm_paths-{layout}"] = lambda pm=pm: h.gbm_paths(S, T, R, SIGMA, Q, N, n, SEED, pm)
            for name, model in JUMPS.items():
                out[f"olmc_jump_paths-{name}-{layout}"] = lambda pm=pm, model=model: h.jump_paths(S, T, R, SIGMA, Q, *model, N, n, SEED, path_major=pm)
                for mirror in (0, 1):
                    out[f"oljd_paths-{name}-mirror{mirror}-{layout}"] = (lambda pm=pm, model=model, mirror=mirror:
                                                                        h.jd_paths(S, T, R, SIGMA, Q, model, N, n, SEED, mirror=bool(mirror), path_major=pm))
    elif group == "heston":
        strikes, steps = cell_sets(n)["3cells"]
        for a in (0, 1):
            out[f"olmc_heston_surface-anti{a}"] = lambda a=a: h.heston_surface(S, T, R, Q, True, *cc.HESTON, strikes, steps, N, n, SEED, bool(a))
            out[f"olmc_heston_qe_surface-anti{a}"] = lambda a=a: h.heston_qe_surface(S, T, R, Q, True, *cc.HESTON, strikes, steps, N, n, SEED, bool(a))
            out[f"olmc_heston_qe_qmc_surface-anti{a}"] = lambda a=a: h.heston_qe_qmc_surface(S, T, R, Q, True, *cc.HESTON, strikes, steps, N, *two(), False, bool(a))
            out[f"olmc_heston_scenarios-anti{a}"] = lambda a=a: h.heston_scenarios(scenarios(), N, n, SEED, bool(a))
            for side, bridge in sides:
                out[f"olmc_heston_qmc_surface-{side}-anti{a}"] = (lambda a=a, bridge=bridge:
                                                                 h.heston_qmc_surface(S, T, R, Q, True, *cc.HESTON, strikes, steps, N, *two(), bridge, bool(a)))
                out[f"olmc_heston_qmc_scenarios-{side}-anti{a}"] = lambda a=a, bridge=bridge: h.heston_qmc_scenarios(scenarios(), N, *two(), bridge, bool(a))
    else:
        raise KeyError(group)
    return out


def hex_words(a):
    """The uint64 words of the doubles, 16 hex digits each, separated by blanks."""
    return " ".join("%016x" % int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel())


def record(label, result):
    """What the fixture keeps of a result: numbers only."""
    if isinstance(result, _hip.Stats):
        return dict(sums=hex_words([result.sum, result.sumsq]), n=int(result.n))
    if isinstance(result, list):
        return [record(label, x) for x in result]
    m = np.ascontiguousarray(result, dtype=np.float64)
    doc = dict(shape=list(m.shape), sha256=hashlib.sha256(m.astype("<f8").tobytes()).hexdigest())
    if label.endswith("path-major"):                                     # a row is a path: n_steps + 1 words
        doc.update(first_row=hex_words(m[0]), last_row=hex_words(m[-1]))
    return doc
