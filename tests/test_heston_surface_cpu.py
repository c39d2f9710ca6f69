"""Host-side checks of the Heston option surface and the calibration on it (no GPU): the refusals that come before the device, the cut of
a surface into launches, the choice of the time grid, implied_volatility against the module's own black_scholes and against the
reference's solver (tests/golden/heston_surface.json), the reference's import lines under compat, the C ABI's refusals."""
import ctypes as C
import itertools
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd import heston as hes
from optionslab_amd.black_scholes import black_scholes, implied_volatility
from optionslab_amd.build import LIBRARY, PROBE_LIBRARY, build_probe_library
from tests.abi_support import library, no_library, _out17 as _out, refused, sobol as _sobol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R, Q = 100.0, 0.05, 0.01
MODEL = (2.0, 0.04, 0.3, -0.7, 0.04)                      # kappa theta sigma_v rho v0
NAMES = ("olmc_heston_surface", "olmc_heston_qmc_surface")


def _market(**over):
    m = dict(spot=S, strikes=(90.0, 100.0, 110.0), maturities=(0.25, 0.5, 1.0), market_ivs=np.full((3, 3), 0.2), r=R, q=Q)
    m.update(over)
    return m


# ------------------------------------------------------------------------------------------------------ the refusals ----
@pytest.mark.parametrize("strikes,maturities,kw,match", [
    ((100.0,), (0.3, 1.0), dict(n_steps=64), "0.3"),                               # 19.2 steps: off the grid, and the message names it
    ((100.0,), (0.5, 1.0), dict(n_steps=63), "0.5"),
    ((100.0,), (0.0, 1.0), dict(n_steps=64), "must be > 0"),
    ((100.0,), (-0.5, 1.0), dict(n_steps=64), "must be > 0"),
    ((100.0,), (float("nan"), 1.0), dict(n_steps=64), "must be > 0"),
    ((100.0,), (), dict(n_steps=64), "maturities"),
    ((), (0.5, 1.0), dict(n_steps=64), "strikes"),
    ((100.0,), (0.5, 1.0), dict(n_steps=64, method="sobol"), "method"),
    ((100.0,), (0.5, 1.0), dict(n_steps=64, method="qmc", path_construction="pca"), "path_construction"),
    ((100.0,), (0.5, 1.0), dict(n_steps=2048, method="qmc"), "1024"),
    ((100.0,), (0.5, 1.0), dict(n_steps=0), ">= 1"),
    ((100.0,), (0.5, 1.0), dict(n_steps=64, n_paths=0), ">= 1"),
])
def test_price_surface_refuses_before_the_device(no_library, strikes, maturities, kw, match):
    with pytest.raises(ValueError, match=match):
        ol.HestonPricer(*MODEL).price_surface(S, strikes, maturities, R, Q, "call", **{"n_paths": 100, **kw})


@pytest.mark.parametrize("market,kw,match", [
    (_market(maturities=(0.3, 0.5, 1.0)), dict(n_steps=64), "0.3"),
    (_market(maturities=(0.0, 0.5, 1.0)), dict(), "positive"),
    (_market(maturities=(0.0, 0.5, 1.0)), dict(n_steps=64), "must be > 0"),
    (_market(strikes=(), market_ivs=np.zeros((0, 3))), dict(), "strikes"),
    (_market(), dict(method="sobol"), "method"),
    (_market(), dict(seed=None), "seed"),
    (_market(market_ivs=np.full((3, 2), 0.2)), dict(), "shape"),
    ({k: v for k, v in _market().items() if k != "market_ivs"}, dict(), "market_ivs"),
    ({k: v for k, v in _market().items() if k not in ("spot", "r")}, dict(), "spot"),
])
def test_calibrate_heston_refuses_before_the_device(no_library, market, kw, match):
    with pytest.raises(ValueError, match=match):
        hes.calibrate_heston(market, **kw)


def test_q_is_optional_in_the_market_data(no_library):
    market = {k: v for k, v in _market().items() if k != "q"}
    assert callable(hes.calibration_objective(market, method="pseudo"))
    assert hes.calibration_objective(market, method="pseudo")((2.0, 0.04, 0.3, -1.5, 0.04)) == 1e10       # a wall: no surface is priced
    assert hes.calibration_objective(market, method="pseudo")((-2.0, 0.04, 0.3, -0.5, 0.04)) == 1e10


# ---------------------------------------------------------------------------------------------- launches and the grid ----
def test_a_surface_is_cut_into_launches_of_at_most_16_cells_sorted_by_step():
    maturities = (0.5, 0.25, 1.0, 0.75, 0.5, 0.125, 1.0)                           # 5 x 7, steps with repeats
    T, steps = hes._surface_steps(maturities, 64)
    assert T == 1.0 and steps == [32, 16, 64, 48, 32, 8, 64]
    launches = hes._surface_launches(steps, 5)
    assert [len(launch) for launch in launches] == [16, 16, 3]
    flat = [cell for launch in launches for cell in launch]
    assert sorted(flat) == sorted(itertools.product(range(5), range(7))) and len(set(flat)) == 35         # every cell once
    walked = [steps[j] for _i, j in flat]
    assert walked == sorted(walked)                                                # by step over the whole surface, so within each launch
    assert [steps[launch[-1][1]] for launch in launches] == [32, 64, 64]           # where each launch's step loop ends
    assert hes._surface_launches([3], 1) == [[(0, 0)]]
    assert [len(launch) for launch in hes._surface_launches([1, 2], 8)] == [16]


def test_the_surface_reaches_the_bindings_launch_by_launch(no_library, monkeypatch):
    calls = []

    def recorder(name):
        def call(*args):
            calls.append((name, args))
            out = []
            for k, m in zip(args[10], args[11]):
                st = _hip.Stats()
                st.price, st.std_error = k + m, 0.5
                out.append(st)
            return out
        return call

    for name in ("heston_surface", "heston_qmc_surface"):
        monkeypatch.setattr(_hip, name, recorder(name))
    strikes, maturities = (80.0, 90.0, 100.0, 110.0, 120.0), (0.5, 0.25, 1.0, 0.75, 0.5, 0.125, 1.0)
    steps = [32, 16, 64, 48, 32, 8, 64]
    p = ol.HestonPricer(*MODEL)
    prices, errors = p.price_surface(S, strikes, maturities, R, Q, "put", 1000, 64, 5, True, True)
    assert prices.shape == (5, 7) and np.all(errors == 0.5)
    assert np.array_equal(prices, np.add.outer(np.array(strikes), np.array(steps, dtype=float)))           # each answer lands in its cell
    assert [name for name, _a in calls] == ["heston_surface"] * 3
    for _name, args in calls:
        assert args[:10] == (S, 1.0, R, Q, False, *MODEL) and args[12:] == (1000, 64, 5, True)      # the same T, n_steps, seed every time
        assert len(args[10]) == len(args[11]) <= 16 and list(args[11]) == sorted(args[11])
    calls.clear()
    p.price_surface(S, strikes[:2], maturities[:3], R, Q, "call", 128, 64, 5, method="qmc", path_construction="sequential")
    (name, args), = calls
    assert name == "heston_qmc_surface" and args[12] == 128 and args[13].shape == (128, 30) and args[15:] == (False, False)


def test_the_default_grid_has_64_steps_a_year_and_holds_every_maturity():
    assert hes._grid_steps((0.25, 0.5, 1.0)) == 64
    assert hes._grid_steps((1.0, 0.25, 0.5, 0.25)) == 64
    assert hes._grid_steps((0.5, 2.0)) == 128 and hes._grid_steps((0.25,)) == 16 and hes._grid_steps((1.0 / 3.0, 1.0)) == 66
    # (0.25, 1/3, 0.9) lies on the grid of 108 steps (dt = 1 / 120: steps 30, 40 and 108), the smallest one from 58 steps up
    assert hes._grid_steps((0.25, 1.0 / 3.0, 0.9)) == 108 and hes._surface_steps((0.25, 1.0 / 3.0, 0.9), 108)[1] == [30, 40, 108]
    # no grid of at most 1024 steps holds maturities in an irrational ratio, or in a ratio with too large a denominator
    for maturities in ((0.25, 1.0 / math.pi, 0.9), (0.25, 1.0 / 3.0, 0.9001), (1.0 / 1031.0, 1.0)):
        with pytest.raises(ValueError, match="no grid"):
            hes._grid_steps(maturities)


# ------------------------------------------------------------------------------------------------ implied volatility ----
def test_implied_volatility_round_trips_black_scholes():
    worst = 0.0
    for strike in (80.0, 90.0, 100.0, 110.0, 120.0):
        for T in (0.25, 0.5, 1.0, 2.0):
            for vol in (0.1, 0.2, 0.35, 0.6):
                for option_type in ("call", "put"):
                    price = black_scholes(S, strike, T, R, vol, option_type, Q)
                    if price < 1e-6:                        # the price no longer tells the volatility to 1e-8 (vega / price ~ 1e-4 here)
                        continue
                    got = implied_volatility(price, S, strike, T, R, option_type, Q)
                    worst = max(worst, abs(got - vol))
                    assert got == pytest.approx(vol, abs=1e-8), (strike, T, vol, option_type)
    print("worst round trip", worst)


def test_implied_volatility_agrees_with_the_reference_solver():
    with open(os.path.join(ROOT, "tests", "golden", "heston_surface.json")) as f:
        doc = json.load(f)
    inp, section = doc["inputs"], doc["implied_vols"]
    assert section["tolerance"] == 1e-8 and len(section["rows"]) == 18
    for row in section["rows"]:
        got = implied_volatility(row["price"], inp["S"], row["strike"], row["maturity"], inp["r"], "call", inp["q"])
        assert abs(got - row["implied_vol"]) <= section["tolerance"], row


def test_implied_volatility_refuses_what_the_reference_refuses():
    for price in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="positive"):
            implied_volatility(price, S, 100.0, 1.0, R)
    for bad in (dict(S=0.0), dict(K=-1.0), dict(T=0.0)):
        args = dict(S=S, K=100.0, T=1.0)
        args.update(bad)
        with pytest.raises(ValueError, match="S, K, T must be positive"):
            implied_volatility(5.0, args["S"], args["K"], args["T"], R)
    with pytest.raises(ValueError, match="below intrinsic"):
        implied_volatility(15.0, S, 80.0, 1.0, R)                                    # a call worth at least 100 - 80 e^{-0.05} = 23.9
    with pytest.raises(ValueError, match="below intrinsic"):
        implied_volatility(1.0, S, 120.0, 1.0, R, "put")
    with pytest.raises(ValueError, match="Could not find implied volatility: Price too high"):
        implied_volatility(99.0, S, 100.0, 1.0, R)                                   # above the price at 500 % volatility
    within = black_scholes(S, 80.0, 1.0, R, 0.001, "call") - 5e-9                     # inside the tolerance under the intrinsic value,
    with pytest.raises(ValueError, match="Could not find implied volatility: Price too low"):       # below the price at 0.1 % volatility
        implied_volatility(within, S, 80.0, 1.0, R)


# ---------------------------------------------------------------------------------------------------------- compat ----
def test_the_references_import_lines_resolve_under_compat():
    code = ("import optionslab_amd.compat as compat; compat.install()\n"
            "from src.pricing_models.heston import HestonPricer, calibrate_heston\n"
            "from src.pricing_models import implied_volatility\n"
            "from src.pricing_models import calibrate_heston as from_package\n"
            "from src.pricing_models.iv_solver import implied_volatility as from_module\n"
            "import optionslab_amd as ol\n"
            "assert calibrate_heston is ol.calibrate_heston is from_package and HestonPricer is ol.HestonPricer\n"
            "assert implied_volatility is ol.implied_volatility is from_module\n"
            "assert abs(implied_volatility(10.450583572185565, 100, 100, 1.0, 0.05) - 0.2) < 1e-8\n"
            "compat.uninstall()\n"
            "import sys; assert 'src.pricing_models.iv_solver' not in sys.modules\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ------------------------------------------------------------------------------------------------------------ the ABI ----
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bT (olmc_[a-z0-9_]+)", out))


def test_the_header_declares_the_bindings_bind_and_both_libraries_export_the_entry_points(library):
    with open(os.path.join(ROOT, "include", "olmc.h")) as f:
        header = f.read()
    build_probe_library()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and header.count(name) >= 2          # declared, and named in the v6 list
        assert name in _hip.PROTOTYPES and hasattr(library, name)
        assert name in _exported(LIBRARY) and name in _exported(PROBE_LIBRARY)
    assert "#define OLMC_ABI_VERSION 6 " in header
    assert library.olmc_abi_version() == 6


def _cells(strikes=(90.0, 100.0), steps=(2, 4)):
    return (C.c_double * len(strikes))(*strikes), (C.c_int32 * len(steps))(*steps), len(strikes)


_HEAD = (100.0, 1.0, 0.05, 0.01, 1, 2.0, 0.04, 0.3)                                  # S T r q is_call kappa theta sigma_v (rho, v0 follow)
_MANY = ((100.0,) * 17, (1,) * 17)
_REFUSALS = [
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 100, 4, 1, 0, None), "null pointer"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, None, _cells()[1], 2, 0, 100, 4, 1, 0, _out()), "null pointer"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, _cells()[0], None, 2, 0, 100, 4, 1, 0, _out()), "null pointer"),
    ("olmc_heston_surface", lambda: (*_HEAD, 1.5, 0.04, *_cells(), 0, 100, 4, 1, 0, _out()), "rho must be in [-1, 1]"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 0, 4, 1, 0, _out()), "n_paths must be >= 1"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 100, 0, 1, 0, _out()), "n_steps must be >= 1"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), -1, 100, 4, 1, 0, _out()), "path_offset must be >= 0"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells()[:2], 0, 0, 100, 4, 1, 0, _out()), "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(*_MANY), 0, 100, 4, 1, 0, _out()), "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(steps=(2, 5)), 0, 100, 4, 1, 0, _out()), "a cell's step must be in [1, n_steps]"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(steps=(0, 4)), 0, 100, 4, 1, 0, _out()), "a cell's step must be in [1, n_steps]"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 0, 64, 4, *_sobol(8), 30, 0, None), "null pointer"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, None, _cells()[1], 2, 0, 0, 64, 4, *_sobol(8), 30, 0, _out()), "null pointer"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 0, 64, 4, None, None, 30, 0, _out()), "null pointer"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -1.5, 0.04, *_cells(), 0, 0, 64, 4, *_sobol(8), 30, 0, _out()), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 2, 0, 64, 4, *_sobol(8), 30, 0, _out()), "bad construction"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 1, 0, 64, 1025, *_sobol(1), 30, 0, _out()),
     "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 0, 64, 0, *_sobol(1), 30, 0, _out()),
     "n_steps must be in [1, 10600]: a step takes two of the 21201 Sobol dimensions"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 0, 64, 4, *_sobol(8), 32, 0, _out()),
     "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(), 0, 0, 0, 4, *_sobol(8), 30, 0, _out()), "n_paths must be >= 1"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells()[:2], 17, 0, 0, 64, 4, *_sobol(8), 30, 0, _out()),
     "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(steps=(5, 1)), 1, 0, 64, 4, *_sobol(8), 30, 0, _out()),
     "a cell's step must be in [1, n_steps]"),
    # two faults at once: the model, then the Sobol call, then the cells
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells()[:2], 0, 2, 0, 64, 4, *_sobol(8), 30, 0, _out()), "bad construction"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -1.5, 0.04, *_cells()[:2], 0, 2, 0, 64, 4, *_sobol(8), 30, 0, _out()), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells()[:2], 17, 0, 0, 64, 4, *_sobol(8), 32, 0, _out()),
     "only 30-bit Sobol tables (SciPy's default) are supported"),
    # Philox: the model, then the range (count, steps, offset), then the cells
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells(steps=(2, 5)), 0, 0, 4, 1, 0, _out()), "n_paths must be >= 1"),
    ("olmc_heston_surface", lambda: (*_HEAD, -0.7, 0.04, *_cells()[:2], 17, 0, 100, 0, 1, 0, _out()), "n_steps must be >= 1"),
    ("olmc_heston_surface", lambda: (*_HEAD, 1.5, 0.04, *_cells(steps=(2, 5)), 0, 0, 4, 1, 0, _out()), "rho must be in [-1, 1]"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    """Each refusal answers OLMC_ERR_ARG (1) with its exact message, ahead of any device work (no device is initialised here)."""
    refused(library, getattr(library, name)(*args()), message)


def test_the_bindings_check_the_cell_lists(no_library):
    with pytest.raises(ValueError, match="one length"):
        _hip.heston_surface(S, 1.0, R, Q, True, *MODEL, [90.0, 100.0], [1], 100, 4, 1)
    sv, shift = np.ones((7, 30), np.uint32), np.zeros(7, np.uint32)
    with pytest.raises(ValueError, match="even"):
        _hip.heston_qmc_surface(S, 1.0, R, Q, True, *MODEL, [90.0], [1], 64, sv, shift)
