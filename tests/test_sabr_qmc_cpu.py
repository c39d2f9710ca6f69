"""CPU checks of SABR on Sobol paths (include/olmc_sabr_qmc.h, optionslab_amd.SABRModelQMC).

  ABI        olmc_sabr_qmc.h's declarations = the library's olsq_* exports = _hip.SABRQ_PROTOTYPES, disjoint from every other table; the
             header is C99; every refusal answers OLMC_ERR_ARG with its exact message, in the header's order (the model before F, F
             before the payoff, the payoff before the points, the points before the cells), before any device is touched.
  Python     SABRModelQMC is exported and keeps SABRModel's signatures; the ValueErrors come before the library is loaded.
  oracle     tests/sabr_qmc_oracle.paths, fed z / z_scale as raw normals, is tests/sabr_oracle.paths within 1e-15 (n + 2) with the same
             zeros; nu = 0, beta = 1 is a GBM recursion; the mirror of the mirror is the path.
  conditions what tests/test_gpu_sabr_qmc.py rests on, for every CASE, both constructions and both legs: no pre-clamp |G| below 1e-7, no
             live state within 1e-9 of a level in log space, each absorbing model absorbs at least 2 % of its 4133-point case; the same
             two guards at the extra shapes the GPU module uses.
  Black-76   at nu = 0, beta = 1, alpha = 0.25, 2^14 x 16 and the bridge the oracle's European price is within 1e-3 of Black-76.
"""
import ctypes as C
import inspect
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import path_draw_oracle as pdo
from tests import sabr_oracle as so
from tests import sabr_qmc_oracle as sq
from tests.abi_support import assert_header_matches, library, no_library, refused, sobol  # noqa: F401  (fixtures)
from tests.test_sabr_cpu import BAD_MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc_sabr_qmc.h")
NAMES = ["olsq_paths", "olsq_price", "olsq_surface_prices"]
BRIDGE_CAP = "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"
STEP_RANGE = "n_steps must be in [1, 10600]: a step takes two of the 21201 Sobol dimensions"
BITS = "only 30-bit Sobol tables (SciPy's default) are supported"
TOO_BIG = "path matrix would exceed 64 GB: lower n_paths or n_steps"

pytestmark = pytest.mark.filterwarnings("ignore:The balance properties of Sobol")


# --------------------------------------------------------------------------------------------------------------- ABI ----
def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "olsq_", _hip.SABRQ_PROTOTYPES, NAMES)
    for other in (_hip.PROTOTYPES, _hip.LV_PROTOTYPES, _hip.LVQ_PROTOTYPES, _hip.JD_PROTOTYPES, _hip.JS_PROTOTYPES, _hip.SABR_PROTOTYPES,
                  _hip.HA_PROTOTYPES):
        assert not set(_hip.SABRQ_PROTOTYPES) & set(other)


def test_header_is_c99(tmp_path):
    from optionslab_amd.build import _hipcc

    cc = shutil.which("gcc") or shutil.which("cc")
    compiler = [cc] if cc else [_hipcc(), "-x", "c"]
    src = tmp_path / "use_header.c"
    src.write_text('#include "olmc_sabr_qmc.h"\n'
                   "int use(const olsb_model* m, const uint32_t* sv, const uint32_t* shift, olmc_stats* out) {\n"
                   "    return olsq_price(100, 100, 1, 0.03, 1, m, OLSB_EUROPEAN, 0, OLMC_QMC_BRIDGE, 0, 1000, 8, sv, shift, 30, 0, out); }\n")
    subprocess.run([*compiler, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use_header.o")], check=True)


def entry_calls(library, m, *, F=100.0, payoff=8, barrier=0.0, construction=1, offset=0, n=100, steps=4, k=2, bits=30, out=True, cells=True,
                sv=True, shift=True):
    """The three entry points on the model pointer m, as thunks that give the return code.  The tables are stand-ins: never read."""
    st = _hip.Stats()
    sts = (_hip.Stats * 16)()
    strikes, cell_steps = (C.c_double * 16)(*([100.0] * 16)), (C.c_int32 * 16)(*([1] * 16))
    fwd, vol = (C.c_double * 8)(), (C.c_double * 8)()
    tsv, tshift = sobol(8)
    psv, psh = tsv if sv else None, tshift if shift else None
    return {
        "olsq_price": lambda: library.olsq_price(F, 100.0, 1.0, 0.03, 1, m, payoff, barrier, construction, offset, n, steps, psv, psh, bits, 0,
                                                 C.byref(st) if out else None),
        "olsq_paths": lambda: library.olsq_paths(F, 1.0, m, construction, n, steps, psv, psh, bits, 0, 1, fwd if out else None, vol),
        "olsq_surface_prices": lambda: library.olsq_surface_prices(F, 1.0, 0.03, 1, m, strikes if cells else None, cell_steps, k, construction, offset,
                                                                   n, steps, psv, psh, bits, 0, sts if out else None),
    }


@pytest.mark.parametrize("entry", NAMES)
def test_every_refusal_answers_its_message_before_any_device_work(library, entry):
    """rc 1 (OLMC_ERR_ARG) and the exact words, on a machine with or without a device: none of these calls initialises one."""
    good = _hip.sabr_model(0.25, 0.5, -0.3, 0.4)
    call = lambda m=C.byref(good), **kw: entry_calls(library, m, **kw)[entry]()
    # 1: pointers, the model and F -- olsb_*'s refusals
    refused(library, call(m=None), "null pointer")
    refused(library, call(out=False), "null pointer")
    if entry == "olsq_surface_prices":
        refused(library, call(cells=False), "null pointer")
    for params, message in BAD_MODELS:
        bad = _hip.sabr_model(*params)
        refused(library, call(m=C.byref(bad), F=-1.0, n=0, payoff=9, construction=2), message)      # the model before F, the payoff and the points
    refused(library, call(F=0.0, n=0, payoff=9, construction=2), "F must be positive")             # F before the payoff and the points
    refused(library, call(F=-3.0), "F must be positive")
    for edge in ((1e-300, 0.0, -1.0, 0.0), (0.2, 1.0, 1.0, 0.0)):                                  # the closed ends of every range are served
        ok = _hip.sabr_model(*edge)
        refused(library, call(m=C.byref(ok), n=0), "n_paths must be >= 1")
    # 2: the payoff
    if entry == "olsq_price":
        refused(library, call(payoff=-1), "bad payoff")
        refused(library, call(payoff=9), "bad payoff")
        for kind in range(4):
            refused(library, call(payoff=kind, barrier=0.0), "Barrier must be positive")
            refused(library, call(payoff=kind, barrier=-5.0), "Barrier must be positive")
        refused(library, call(payoff=9, barrier=-5.0), "bad payoff")
        refused(library, call(payoff=9, construction=2, steps=0), "bad payoff")                    # the payoff before the points
        refused(library, call(payoff=0, barrier=0.0, bits=32, n=0), "Barrier must be positive")
    # 3: the construction, the tables and the points -- olmc_heston_qmc's refusals
    refused(library, call(construction=2), "bad construction")
    refused(library, call(construction=-1), "bad construction")
    refused(library, call(steps=1025), BRIDGE_CAP)
    refused(library, call(steps=10601), BRIDGE_CAP)
    refused(library, call(steps=10601, construction=0), STEP_RANGE)
    refused(library, call(steps=0), STEP_RANGE)
    refused(library, call(steps=-4, construction=0), STEP_RANGE)
    refused(library, call(sv=False), "null pointer")
    refused(library, call(shift=False), "null pointer")
    refused(library, call(bits=32), BITS)
    refused(library, call(n=0), "n_paths must be >= 1")
    refused(library, call(n=(1 << 30) + 1, steps=1), "at most 2**30 Sobol points")
    if entry != "olsq_paths":
        refused(library, call(offset=-1), "path_offset must be >= 0")
        refused(library, call(offset=1 << 30, n=1), "at most 2**30 Sobol points")
    refused(library, call(construction=2, steps=1025, bits=32), "bad construction")                # in SobolCall's own order
    refused(library, call(steps=1025, sv=False), BRIDGE_CAP)
    refused(library, call(steps=0, sv=False), STEP_RANGE)
    refused(library, call(sv=False, bits=32), "null pointer")
    refused(library, call(bits=32, n=0), BITS)
    refused(library, call(n=0, offset=-1), "n_paths must be >= 1")
    # 4: the cells, after the points
    if entry == "olsq_surface_prices":
        refused(library, call(k=0), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        refused(library, call(k=17), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        refused(library, call(k=17, bits=32), BITS)
        refused(library, call(k=0, construction=2), "bad construction")
        sts = (_hip.Stats * 2)()
        tsv, tshift = sobol(8)
        strikes, steps = (C.c_double * 2)(100.0, 100.0), (C.c_int32 * 2)(1, 5)
        refused(library, library.olsq_surface_prices(100.0, 1.0, 0.03, 1, C.byref(good), strikes, steps, 2, 1, 0, 100, 4, tsv, tshift, 30, 0, sts),
                "a cell's step must be in [1, n_steps]")
    if entry == "olsq_paths":
        refused(library, call(n=1 << 30, steps=8), TOO_BIG)
        refused(library, call(n=1 << 30, steps=8, construction=2), "bad construction")
        refused(library, call(n=1 << 30, steps=8, bits=32), BITS)


# ------------------------------------------------------------------------------------------------------------ Python ----
METHODS = ("price_monte_carlo", "simulate_paths", "price_asian", "price_barrier", "price_lookback", "price_surface", "smile_monte_carlo", "price",
           "implied_vol", "smile")


def test_python_surface_of_the_qmc_model():
    assert "SABRModelQMC" in ol.__all__ and ol.SABRModelQMC is ol.sabr.SABRModelQMC and issubclass(ol.SABRModelQMC, ol.SABRModel)
    for name in METHODS:
        assert inspect.signature(getattr(ol.SABRModelQMC, name)) == inspect.signature(getattr(ol.SABRModel, name)), name
    assert list(inspect.signature(ol.SABRModelQMC).parameters) == ["alpha", "beta", "rho", "nu", "path_construction"]
    assert list(inspect.signature(ol.SABRModel.qmc).parameters) == ["self", "path_construction"]
    assert inspect.signature(ol.SABRModel.qmc).parameters["path_construction"].default == "bridge"
    model = ol.SABRModel(0.25, 0.5, -0.3, 0.4)
    for construction in ("bridge", "sequential"):
        view = model.qmc(construction)
        assert type(view) is ol.SABRModelQMC and view.path_construction == construction and view._model() == model._model()
        assert view.price(100.0, 95.0, 1.0, 0.03) == model.price(100.0, 95.0, 1.0, 0.03)             # Hagan's side is untouched
    assert model.qmc().path_construction == "bridge"
    assert set(_hip.SABRQ_PROTOTYPES) == set(NAMES) and all(callable(getattr(_hip, f)) for f in ("sabrq_price", "sabrq_paths", "sabrq_surface_prices"))
    with pytest.raises(ValueError, match="alpha must be positive"):
        ol.SABRModelQMC(0.0, 0.5, 0.0, 0.4)


def test_python_refusals_come_before_the_library_is_loaded(no_library):
    model = ol.SABRModel(0.25, 0.5, -0.3, 0.4)
    with pytest.raises(ValueError, match="path_construction"):
        model.qmc("spiral")
    with pytest.raises(ValueError, match="path_construction"):
        ol.SABRModelQMC(0.25, 0.5, -0.3, 0.4, path_construction="spiral")
    view, seq = model.qmc(), model.qmc("sequential")
    with pytest.raises(ValueError, match="at most 10600 steps"):
        seq.price_monte_carlo(100, 100, 1.0, 0.03, n_paths=16, n_steps=10601, seed=1)
    with pytest.raises(ValueError, match="at most 10600 steps"):
        view.price_surface(100, [100.0], [1.0], 0.03, n_paths=16, n_steps=10601, seed=1)
    with pytest.raises(ValueError, match="at most 1024 steps"):
        view.price_asian(100, 100, 1.0, 0.03, n_paths=16, n_steps=1025, seed=1)
    with pytest.raises(ValueError, match="at most 1024 steps"):
        view.simulate_paths(100, 1.0, n_paths=16, n_steps=1025, seed=1)
    with pytest.raises(ValueError, match="2\\*\\*30"):
        view.price_lookback(100, 100, 1.0, 0.03, n_paths=(1 << 30) + 1, n_steps=4, seed=1)
    refusals = [
        lambda: view.price_monte_carlo(100, 100, 1.0, 0.03, n_paths=0), lambda: view.simulate_paths(100, 1.0, n_paths=0),
        lambda: view.price_monte_carlo(0.0, 100, 1.0, 0.03), lambda: view.price_monte_carlo(-1.0, 100, 1.0, 0.03),
        lambda: view.simulate_paths(0.0, 1.0), lambda: view.price_surface(0.0, [100.0], [1.0], 0.03), lambda: view.smile_monte_carlo(0.0, 1.0, [100.0]),
        lambda: view.smile_monte_carlo(100, 1.0, [100.0], n_paths=0), lambda: view.price_barrier(100, 100, 1.0, 0.03, 0.0),
        lambda: view.price_asian(100, 100, 1.0, 0.03, avg_type="harmonic"),
    ]
    for refusal in refusals:
        with pytest.raises(ValueError):
            refusal()
    for good in (lambda: view.price_monte_carlo(100, 100, 1.0, 0.03, n_paths=16, n_steps=2, seed=1),
                 lambda: seq.simulate_paths(100, 1.0, n_paths=16, n_steps=2, seed=1),
                 lambda: view.price_surface(100, [100.0], [1.0], 0.03, n_paths=16, n_steps=2, seed=1)):
        with pytest.raises(AssertionError, match="the library was loaded"):                       # the fixture does bite: a good call reaches for it
            good()


# ------------------------------------------------------------------------------------------------------------ oracle ----
def test_cases_are_a_latin_square():
    assert len(sq.CASES) == len(set(sq.CASES)) == 8 * 5
    for n in sq.STEPS + (sq.SEQUENTIAL_ONLY,):
        mine = [c for c in sq.CASES if c[2] == n]
        assert sorted(c[0] for c in mine) == sorted(sq.MODELS) and set(c[1] for c in mine) == set(sq.POINTS)
    for name in sq.MODELS:
        assert {c[1] for c in sq.CASES if c[0] == name} == set(sq.POINTS)
    assert sq.constructions(1024) == (True, False) and sq.constructions(1025) == (False,)
    for name in so.ABSORBING:
        assert any(c[0] == name and c[1] == 4133 for c in sq.CASES)


@pytest.mark.parametrize("name", list(sq.MODELS))
def test_the_oracle_is_the_philox_oracle_on_rescaled_normals(name):
    """Fed z / z_scale as raw normals, tests/sabr_oracle.paths forms z_scale (z / z_scale): the same recursion within rounding."""
    N, n = 257, 13
    z = sq.normals(n, N)
    inv = 1.0 / so.LONG(pdo.z_scale(so.LONG))
    for bridge in (True, False):
        z1, z2 = sq.step_normals(z, bridge)
        for mirror in (False, True):
            got = sq.paths(sq.F0, sq.T, sq.MODELS[name], n, z1, z2, mirror)
            want = so.paths(sq.F0, sq.T, sq.MODELS[name], n, z1.astype(so.LONG) * inv, z2.astype(so.LONG) * inv, mirror)
            assert np.array_equal(got[0] == 0, want[0] == 0), (name, bridge, mirror)
            for a, b in ((got[0], want[0]), (got[1], want[1])):
                live = b != 0
                assert float(np.max(np.abs(a[live] / b[live] - 1))) <= 1e-15 * (n + 2), (name, bridge, mirror)


def test_oracle_without_vol_of_vol_and_beta_one_is_a_gbm_recursion():
    inv = 1.0 / so.LONG(pdo.z_scale(so.LONG))
    for n in (1, 13, 64):
        z = sq.normals(n, 257)
        for bridge in (True, False):
            z1, z2 = sq.step_normals(z, bridge)
            forward, vol, closest = sq.paths(sq.F0, sq.T, (0.25, 1.0, -0.4, 0.0), n, z1, z2)
            want = so.gbm_paths(sq.F0, sq.T, 0.25, n, z1.astype(so.LONG) * inv)
            assert np.all(vol == 0.25) and closest == np.inf
            assert float(np.max(np.abs(forward / want - 1))) <= 1e-15 * (n + 2)


def test_oracle_mirror_of_the_mirror_is_the_path():
    z = sq.normals(13, 65)
    for name, model in sq.MODELS.items():
        for bridge in (True, False):
            z1, z2 = sq.step_normals(z, bridge)
            plain = sq.paths(sq.F0, sq.T, model, 13, z1, z2)
            mirror = sq.paths(sq.F0, sq.T, model, 13, z1, z2, mirror=True)
            back = sq.paths(sq.F0, sq.T, model, 13, -z1, -z2, mirror=True)
            assert np.array_equal(back[0], plain[0]) and np.array_equal(back[1], plain[1]), name
            assert not np.array_equal(mirror[0][:, 1:], plain[0][:, 1:])
            assert np.all(plain[0][:, 0] == sq.F0) and np.all(plain[1][:, 0] == model[0])
    z1, z2 = sq.step_normals(z, True)
    m1, m2 = sq.step_normals(-z, True)
    assert np.array_equal(m1, -z1) and np.array_equal(m2, -z2)                                     # -z gives -W on both bridges, bit for bit


# -------------------------------------------------------------------------------------------------------- conditions ----
def guards(name, N, n, z=None):
    """(smallest pre-clamp |G|, smallest clearance, absorbed fractions) over both constructions and both legs of a shape."""
    z = sq.normals(n, N) if z is None else z
    closest, clearance, absorbed = np.inf, np.inf, []
    for bridge in sq.constructions(n):
        for mirror in (False, True):
            forward, _vol, g = sq.case_paths(name, N, n, bridge, mirror, z)
            closest = min(closest, g)
            clearance = min(clearance, sq.level_clearance(forward.astype(np.float64)))
            absorbed.append(float(np.mean(forward[:, -1] == 0)))
            if sq.MODELS[name][1] == 1.0:
                assert np.all(forward > 0)
    return closest, clearance, absorbed


@pytest.mark.parametrize("name", list(sq.MODELS))
def test_the_gpu_module_s_conditions_hold_for_every_case(name):
    worst = dict(closest=np.inf, clearance=np.inf)
    for _name, N, n in sq.CASES:
        if _name != name:
            continue
        closest, clearance, absorbed = guards(name, N, n)
        worst.update(closest=min(worst["closest"], closest), clearance=min(worst["clearance"], clearance))
        assert closest > 1e-7, (name, N, n, closest)
        assert clearance > 1e-9, (name, N, n, clearance)
        if name in so.ABSORBING and N == 4133:
            print("DEVIATION " + json.dumps(dict(test="absorbed", model=name, n=n, fractions=absorbed)))
            assert min(absorbed) >= 0.02, (name, n, absorbed)
    print("DEVIATION " + json.dumps(dict(test="conditions", model=name, closest_g=None if np.isinf(worst["closest"]) else worst["closest"],
                                         clearance=worst["clearance"])))


@pytest.mark.parametrize("name", list(sq.MODELS))
def test_the_guards_hold_at_the_extra_shapes_of_the_gpu_module(name):
    worst = dict(closest=np.inf, clearance=np.inf)
    for N, n in [(N, 64) for N in sq.POINTS] + [(257, 13), (4133, 13)]:
        closest, clearance, _absorbed = guards(name, N, n)
        worst.update(closest=min(worst["closest"], closest), clearance=min(worst["clearance"], clearance))
        assert closest > 1e-7 and clearance > 1e-9, (name, N, n, closest, clearance)
    print("DEVIATION " + json.dumps(dict(test="extra-shapes", model=name, closest_g=None if np.isinf(worst["closest"]) else worst["closest"],
                                         clearance=worst["clearance"])))


# ---------------------------------------------------------------------------------------------------------- Black-76 ----
def test_the_oracle_s_black_76_case_is_within_a_thousandth():
    assert (sq.BLACK_MODEL, sq.BLACK_POINTS, sq.BLACK_STEPS) == ((0.25, 1.0, -0.4, 0.0), 1 << 14, 16)
    for is_call in (True, False):
        price = sq.black_case_price(is_call)
        black = float(ol.SABRModel._black_price(sq.F0, 100.0, sq.T, sq.R, sq.BLACK_SIGMA, "call" if is_call else "put"))
        print("DEVIATION " + json.dumps(dict(test="black-76-oracle", is_call=is_call, price=price, closed_form=black, gap=abs(price - black))))
        assert abs(price - black) <= 1e-3
