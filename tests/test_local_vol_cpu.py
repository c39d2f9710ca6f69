"""CPU checks of the Dupire local-volatility family (include/olmc_local_vol.h, optionslab_amd/local_vol.py).

  golden   the package's dupire_formula and calibrated surface against tests/golden/local_vol.json, recorded from the reference: 1e-9
           relative (same arithmetic; only the normal CDF's last ulps could differ, which the second difference amplifies by about 1e3 to
           1e-12, while a slip in a difference quotient moves values by 1e-3); floor and fallback cells exactly.
  table    local_vol_table equals the clipped surface at its nodes and is flat beyond the strikes' range.
  oracle   tests/local_vol_oracle.py against closed forms: a flat table is the GBM recursion, a one-step path has a hand-computed lookup.
  ABI      olmc_local_vol.h's declarations = the library's ollv_* exports = _hip.LV_PROTOTYPES; the header is C99; the struct is 40 bytes;
           every refusal answers OLMC_ERR_ARG with its exact message before any device is touched.
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
from tests import local_vol_oracle as lvo
from tests.abi_support import assert_header_matches, library, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc_local_vol.h")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "local_vol.json")))
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def arrays(case):
    return np.array(case["strikes"]), np.array(case["expiries"]), np.array(case["iv"])


@pytest.fixture(scope="module")
def sample():
    """(model, calibrated surface) of the reference's sample surface."""
    case = CASES["sample"]
    model = ol.DupireLocalVol(r=case["r"], q=case["q"])
    return model, model.calibrate(*arrays(case), case["spot"])


# ------------------------------------------------------------------------------------------------------------ golden ----
@pytest.mark.parametrize("name", ["sample", "small_q", "small_q_four_expiries"])
def test_dupire_formula_matches_the_reference(name):
    case = CASES[name]
    strikes, expiries, iv = arrays(case)
    got = ol.DupireLocalVol(r=case["r"], q=case["q"]).dupire_formula(strikes, expiries, iv, case["spot"])
    want = np.array(case["local_vol"])
    assert got.shape == want.shape == iv.shape
    assert np.max(np.abs(got - want) / want) <= 1e-9
    floor = float(np.sqrt(0.001))
    assert [[int(i), int(j)] for i, j in zip(*np.nonzero(got == floor))] == case["floor_cells"]
    for i, j in case["floor_cells"]:
        assert got[i, j] == want[i, j] == floor
    for i, j in case["fallback_cells"]:
        assert got[i, j] == want[i, j] == iv[i, j]
    assert np.array_equal(got[0, 1:-1], iv[0, 1:-1]) and np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, -1], got[:, -2])


def test_the_sample_surface_is_the_reference_s_and_has_five_floor_cells():
    strikes, expiries, iv = ol.create_sample_iv_surface()
    want = arrays(CASES["sample"])
    assert np.array_equal(strikes, want[0]) and np.array_equal(expiries, want[1]) and np.max(np.abs(iv - want[2])) <= 1e-15
    assert iv.shape == (5, 20) and len(CASES["sample"]["floor_cells"]) == 5


@pytest.mark.parametrize("name", ["sample", "small_q_four_expiries"])
def test_calibrated_surface_matches_the_reference_inside_and_outside_the_nodes(name):
    case = CASES[name]
    surface = ol.DupireLocalVol(r=case["r"], q=case["q"]).calibrate(*arrays(case), case["spot"])
    points = case["surface"]
    lo, hi = case["strikes"][0], case["strikes"][-1]
    assert sum(p["K"] < lo for p in points) >= len(points) // 4 and sum(p["K"] > hi for p in points) >= len(points) // 4
    for p in points:
        assert abs(surface(p["K"], p["T"]) - p["value"]) <= 1e-9 * abs(p["value"]), p
    # the flat continuation the fixture pins: beyond the nodes the surface is its value at the nearest edge
    t_lo, t_hi = case["expiries"][0], case["expiries"][-1]
    for t in (0.05, 0.6, 1.5):
        assert surface(0.5 * lo, t) == pytest.approx(surface(lo, min(max(t, t_lo), t_hi)), rel=1e-12)
        assert surface(2.0 * hi, t) == pytest.approx(surface(hi, min(max(t, t_lo), t_hi)), rel=1e-12)


def test_a_surface_too_small_for_the_spline_is_refused_as_the_reference_refuses_it():
    case = CASES["small_q"]
    assert case["calibrate_raises"] and "surface" not in case          # the reference raised (the class is SciPy's and not pinned here)
    with pytest.raises(Exception):
        ol.DupireLocalVol(r=case["r"], q=case["q"]).calibrate(*arrays(case), case["spot"])


# ------------------------------------------------------------------------------------------------------------- table ----
@pytest.mark.parametrize("S,T,n_x,n_t", [(100.0, 1.0, 128, 33), (95.0, 0.5, 7, 2), (100.0, 1.0, 16, 1)])
def test_table_is_the_clipped_surface_at_its_nodes_and_flat_beyond(sample, S, T, n_x, n_t):
    model, surface = sample
    vol, x_lo, x_hi, t_hi = model.local_vol_table(S, T, n_x, n_t)
    assert vol.shape == (n_t, n_x) and vol.min() >= 0.05 and vol.max() <= 2.0
    assert x_lo == pytest.approx(np.log(70.0 / S), abs=1e-14) and x_hi == pytest.approx(np.log(130.0 / S), abs=1e-14)
    xs = np.linspace(x_lo, x_hi, n_x)
    ts = np.linspace(0.0, t_hi, n_t) if n_t > 1 else [T]
    if n_t > 1:
        assert t_hi == min(T, 1.0)
    for i in sorted({0, n_t // 2, n_t - 1}):
        for j in sorted({0, 1, n_x // 3, n_x - 2, n_x - 1}):
            want = float(np.clip(surface(S * np.exp(xs[j]), ts[i]), 0.05, 2.0))
            assert vol[i, j] == pytest.approx(want, rel=1e-10), (i, j)
    # beyond the strikes' range the kernels' flat edge and the surface's flat continuation are the same number (to the fp32 rounding of a node)
    table = lvo.Table(vol, x_lo, x_hi, t_hi)
    for tau in (0.0, 0.37 * t_hi, t_hi):
        below, above = table.lookup(np.array([x_lo - 0.5, x_lo - 1e-9]), tau), table.lookup(np.array([x_hi + 1e-9, x_hi + 0.7]), tau)
        assert below[0] == below[1] and above[0] == above[1]
    row = n_t - 1
    t_row = ts[row]
    assert table.lookup(np.array([x_lo - 0.5]), t_row)[0] == pytest.approx(np.clip(surface(S * np.exp(x_lo - 0.5), t_row), 0.05, 2.0), rel=1e-7)
    assert table.lookup(np.array([x_hi + 0.7]), t_row)[0] == pytest.approx(np.clip(surface(S * np.exp(x_hi + 0.7), t_row), 0.05, 2.0), rel=1e-7)


def test_an_uncalibrated_model_prices_on_a_flat_twenty_percent():
    vol, x_lo, x_hi, _t_hi = ol.DupireLocalVol().local_vol_table(100.0, 1.0)
    assert np.all(vol == 0.2) and vol.shape[1] >= 2 and x_hi > x_lo


# ------------------------------------------------------------------------------------------------------------ oracle ----
def test_oracle_flat_table_is_the_gbm_recursion():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((50, 13))
    S, T, r, q, sigma = 100.0, 0.75, 0.05, 0.01, 0.25              # 0.25 is exact in fp32
    for vol in (np.full(2, sigma), np.full((3, 7), sigma)):
        x = lvo.log_paths(z, lvo.Table(vol, -0.3, 0.2, 0.5), T, r, q)
        dt = T / 13
        want = np.concatenate([np.zeros((50, 1)), np.cumsum((r - q - 0.5 * sigma**2) * dt + sigma * np.sqrt(dt) * z, axis=1)], axis=1)
        assert np.max(np.abs(x - want)) <= 1e-14
        assert np.max(np.abs(lvo.gbm_normals(lvo.paths(z, lvo.Table(vol, -0.3, 0.2, 0.5), S, T, r, q), T, r, sigma, q) - z)) <= 1e-11


def test_oracle_lookup_by_hand():
    """A[2][3] with exactly representable nodes over x in [-1, 1], tau in [0, 2]."""
    table = lvo.Table([[0.25, 0.5, 0.75], [0.5, 1.0, 1.5]], -1.0, 1.0, 2.0)
    at = lambda x, tau: float(table.lookup(np.array([x]), tau)[0])
    assert at(-1.0, 0.0) == 0.25 and at(0.0, 0.0) == 0.5 and at(1.0, 2.0) == 1.5             # nodes
    assert at(0.5, 0.0) == 0.625                                                             # u = 1.5: 0.5 + 0.5 (0.75 - 0.5)
    assert at(0.5, 1.0) == 0.9375                                                            # rows 0.625 and 1.25, w_tau = 0.5
    assert at(-0.5, 0.5) == 0.375 + 0.25 * (0.75 - 0.375)                                    # u = 0.5, w_tau = 0.25
    assert at(-7.0, 1.0) == at(-1.0, 1.0) == 0.375 and at(9.0, 1.0) == at(1.0, 1.0) == 1.125    # flat beyond the x edges
    assert at(0.5, 5.0) == at(0.5, 2.0) == 1.25 and at(0.5, -1.0) == at(0.5, 0.0)            # flat beyond the tau edges
    one_row = lvo.Table([0.25, 0.5, 0.75], -1.0, 1.0)
    assert float(one_row.lookup(np.array([0.5]), 123.0)[0]) == 0.625                         # n_t == 1: no time axis


def test_oracle_one_step_path_by_hand():
    table = lvo.Table([[0.25, 0.5, 0.75], [0.5, 1.0, 1.5]], -1.0, 1.0, 2.0)
    S, T, r, q = 100.0, 0.5, 0.04, 0.01
    z = np.array([[1.0, -2.0]])
    x = lvo.log_paths(z, table, T, r, q)
    dt = 0.25
    x1 = (r - q - 0.5 * 0.5**2) * dt + 0.5 * 0.5 * 1.0                         # x_0 = 0 is the middle node of row 0: sigma_0 = 0.5
    u = (x1 + 1.0)                                                             # (x - x_lo) (n_x - 1) / (x_hi - x_lo), in [1, 2]
    a0, a1 = 0.5 + (u - 1) * 0.25, 1.0 + (u - 1) * 0.5
    s1 = a0 + (dt * 1 / 2.0) * (a1 - a0)                                       # tau = dt, v = tau (n_t - 1) / t_hi
    x2 = x1 + (r - q - 0.5 * s1**2) * dt + s1 * 0.5 * -2.0
    assert x[0, 0] == 0.0 and x[0, 1] == pytest.approx(x1, abs=1e-16) and x[0, 2] == pytest.approx(x2, abs=1e-15)
    assert lvo.paths(z, table, S, T, r, q)[0, 0] == S


def test_oracle_payoffs_by_hand():
    spot = np.array([[100.0, 120.0, 90.0, 110.0], [100.0, 95.0, 80.0, 85.0]])
    assert list(lvo.payoff(spot, 0, True, 100.0, 115.0)) == [0.0, 0.0] and list(lvo.payoff(spot, 1, True, 100.0, 115.0)) == [10.0, 0.0]
    assert list(lvo.payoff(spot, 2, False, 100.0, 85.0)) == [0.0, 0.0] and list(lvo.payoff(spot, 3, False, 100.0, 85.0)) == [0.0, 15.0]
    assert list(lvo.payoff(spot, 4, True, 0.0)) == [20.0, 5.0] and list(lvo.payoff(spot, 5, False, 100.0)) == [10.0, 20.0]
    assert lvo.payoff(spot, 6, True, 100.0)[0] == pytest.approx(20.0 / 3) and lvo.payoff(spot, 8, False, 100.0)[1] == 15.0
    assert lvo.payoff(spot, 7, True, 100.0)[0] == pytest.approx((120.0 * 90.0 * 110.0) ** (1 / 3) - 100.0)


# --------------------------------------------------------------------------------------------------------------- ABI ----
def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "ollv_", _hip.LV_PROTOTYPES, ["ollv_paths", "ollv_price", "ollv_surface_prices"])


def test_header_is_c99_and_the_struct_is_forty_bytes(tmp_path):
    assert C.sizeof(_hip.LvSurface) == 40 and _hip.LvSurface.x_lo.offset == 16 and _hip.LvSurface.t_hi.offset == 32
    from optionslab_amd.build import _hipcc

    cc = shutil.which("gcc") or shutil.which("cc")
    compiler = [cc] if cc else [_hipcc(), "-x", "c"]                 # the library was built, so hipcc's clang is there: never skipped
    src = tmp_path / "use_header.c"
    src.write_text('#include "olmc_local_vol.h"\n'
                   "typedef char surface_is_40_bytes[sizeof(ollv_surface) == 40 ? 1 : -1];\n"
                   "typedef char european_is_8[OLLV_EUROPEAN == 8 && OLMC_PATH_ASIAN_GEOMETRIC == 7 ? 1 : -1];\n"
                   "int use(const ollv_surface* s, olmc_stats* out) { return ollv_price(100, 100, 1, 0.05, 0, 1, s, OLLV_EUROPEAN, 0, 0, 1000, 8, 1, 0, out); }\n")
    subprocess.run([*compiler, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use_header.o")], check=True)


def surface(vol=((0.2, 0.3), (0.25, 0.35)), x_lo=-0.5, x_hi=0.5, t_hi=1.0, n_x=None, n_t=None):
    vol = np.ascontiguousarray(vol, dtype=np.float64)
    s = _hip.LvSurface(vol.ctypes.data_as(C.POINTER(C.c_double)), vol.shape[1] if n_x is None else n_x, vol.shape[0] if n_t is None else n_t,
                       x_lo, x_hi, t_hi)
    return s, vol


BAD_SURFACES = [
    (dict(n_x=1), "n_x must be in [2, 256]"), (dict(n_x=257), "n_x must be in [2, 256]"),
    (dict(n_t=0), "n_t must be in [1, 64]"), (dict(n_t=65), "n_t must be in [1, 64]"),
    (dict(x_lo=0.5, x_hi=0.5), "x_hi must be > x_lo"), (dict(x_lo=0.5, x_hi=-0.5), "x_hi must be > x_lo"), (dict(x_hi=float("nan")), "x_hi must be > x_lo"),
    (dict(t_hi=0.0), "t_hi must be > 0"), (dict(t_hi=float("nan")), "t_hi must be > 0"),
    (dict(vol=((0.2, 0.0), (0.2, 0.2))), "local volatilities must be finite and > 0"),
    (dict(vol=((0.2, -0.1), (0.2, 0.2))), "local volatilities must be finite and > 0"),
    (dict(vol=((0.2, 0.2), (float("nan"), 0.2))), "local volatilities must be finite and > 0"),
    (dict(vol=((0.2, 0.2), (0.2, float("inf")))), "local volatilities must be finite and > 0"),
    (dict(vol=((0.2, 1e-60), (0.2, 0.2))), "local volatilities must be finite and > 0"),       # 0 once rounded to fp32
]


def entry_calls(library, s, *, payoff=8, barrier=0.0, offset=0, n=100, steps=4, k=2, out=True, cells=True, matrix=True):
    """The three entry points on the surface pointer s, as thunks that give the return code."""
    st = _hip.Stats()
    sts = (_hip.Stats * 16)()
    strikes, cell_steps = (C.c_double * 16)(*([100.0] * 16)), (C.c_int32 * 16)(*([1] * 16))
    buf = (C.c_double * 8)()
    return {
        "ollv_price": lambda: library.ollv_price(100.0, 100.0, 1.0, 0.05, 0.0, 1, s, payoff, barrier, offset, n, steps, 7, 0, C.byref(st) if out else None),
        "ollv_paths": lambda: library.ollv_paths(100.0, 1.0, 0.05, 0.0, s, n, steps, 7, 1, buf if matrix else None),
        "ollv_surface_prices": lambda: library.ollv_surface_prices(100.0, 1.0, 0.05, 0.0, 1, s, strikes if cells else None, cell_steps, k, offset, n, steps,
                                                                   7, 0, sts if out else None),
    }


@pytest.mark.parametrize("entry", sorted(_hip.LV_PROTOTYPES))
def test_every_refusal_answers_its_message_before_any_device_work(library, entry):
    """rc 1 (OLMC_ERR_ARG) and the exact words, on a machine with or without a device: none of these calls initialises one."""
    good, keep = surface()
    call = lambda s=C.byref(good), **kw: entry_calls(library, s, **kw)[entry]()
    refused(library, call(s=None), "null pointer")
    null_vol = _hip.LvSurface(None, 2, 2, -0.5, 0.5, 1.0)
    refused(library, call(s=C.byref(null_vol)), "null pointer")
    refused(library, call(out=False, matrix=False), "null pointer")
    if entry == "ollv_surface_prices":
        refused(library, call(cells=False), "null pointer")
    for kw, message in BAD_SURFACES:
        bad, keep_bad = surface(**kw)
        refused(library, call(s=C.byref(bad)), message)
    one_row, keep_row = surface(vol=((0.2, 0.3),), t_hi=float("nan"))          # t_hi is unread when n_t == 1: not refused for it
    refused(library, call(s=C.byref(one_row), n=0), "n_paths must be >= 1")
    refused(library, call(n=0), "n_paths must be >= 1")
    refused(library, call(steps=0), "n_steps must be >= 1")
    if entry != "ollv_paths":
        refused(library, call(offset=-1), "path_offset must be >= 0")
    if entry == "ollv_price":
        refused(library, call(payoff=-1), "bad payoff")
        refused(library, call(payoff=9), "bad payoff")
        for kind in range(4):
            refused(library, call(payoff=kind, barrier=0.0), "Barrier must be positive")
            refused(library, call(payoff=kind, barrier=-5.0), "Barrier must be positive")
    if entry == "ollv_surface_prices":
        refused(library, call(k=0), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        refused(library, call(k=17), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        sts = (_hip.Stats * 2)()
        strikes, steps = (C.c_double * 2)(100.0, 100.0), (C.c_int32 * 2)(1, 5)
        refused(library, library.ollv_surface_prices(100.0, 1.0, 0.05, 0.0, 1, C.byref(good), strikes, steps, 2, 0, 100, 4, 7, 0, sts),
                "a cell's step must be in [1, n_steps]")
    if entry == "ollv_paths":
        refused(library, call(n=1 << 33, steps=1), "path matrix would exceed 64 GB")
    # two faults at once: the payoff before the range, inside the range the count before the steps, the range before the cells and the size
    if entry == "ollv_price":
        refused(library, call(payoff=9, steps=0), "bad payoff")
        refused(library, call(payoff=0, barrier=0.0, n=0), "Barrier must be positive")
    if entry == "ollv_surface_prices":
        refused(library, library.ollv_surface_prices(100.0, 1.0, 0.05, 0.0, 1, C.byref(good), strikes, steps, 2, 0, 0, 4, 7, 0, sts),
                "n_paths must be >= 1")
        refused(library, call(k=17, steps=0), "n_steps must be >= 1")
    if entry == "ollv_paths":
        refused(library, call(n=0, steps=0), "n_paths must be >= 1")
        refused(library, call(n=1 << 33, steps=0), "n_steps must be >= 1")
    assert keep is not None and keep_bad is not None and keep_row is not None


# ------------------------------------------------------------------------------------------------------------ Python ----
def test_python_surface_of_the_model():
    assert ol.DupireLocalVol is ol.local_vol.DupireLocalVol and "DupireLocalVol" in ol.__all__ and "create_sample_iv_surface" in ol.__all__
    sig = inspect.signature(ol.DupireLocalVol.__init__)
    assert [p for p in sig.parameters][1:] == ["r", "q", "n_paths", "n_steps", "seed"]
    assert sig.parameters["n_paths"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["n_paths"].default == 100_000
    assert list(inspect.signature(ol.DupireLocalVol.price).parameters) == ["self", "S", "K", "T", "r", "sigma", "option_type", "q"]
    for name in ("price_monte_carlo", "price_asian", "price_barrier", "price_lookback", "price_surface"):
        want = [p for p in inspect.signature(getattr(ol.HestonPricer, name)).parameters if p not in ("method", "path_construction", "scheme")]
        assert list(inspect.signature(getattr(ol.DupireLocalVol, name)).parameters) == want, name
    assert list(inspect.signature(ol.DupireLocalVol.simulate_paths).parameters) == ["self", "S", "T", "r", "q", "n_paths", "n_steps", "seed"]
    assert not hasattr(ol.DupireLocalVol, "price_fdm")
    model = ol.DupireLocalVol()
    with pytest.raises(ValueError):
        model.price_barrier(100, 100, 1.0, 0.05, 0.0)
    with pytest.raises(ValueError):
        model.price_asian(100, 100, 1.0, 0.05, avg_type="harmonic")
    with pytest.raises(ValueError):
        model.price_lookback(100, 100, 1.0, 0.05, lookback_type="partial")
    with pytest.raises(ValueError):
        model.price_monte_carlo(100, 100, 1.0, 0.05, n_paths=0)
    with pytest.raises(ValueError):
        model.price_surface(100, [100.0], [0.3, 1.0], 0.05, n_steps=4)


def test_compat_serves_the_reference_import_path():
    import sys

    import optionslab_amd.compat as compat

    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    try:
        compat.install()
        from src.pricing_models.local_vol import DupireLocalVol, LocalVolSurface, create_sample_iv_surface
        assert DupireLocalVol is ol.DupireLocalVol and LocalVolSurface is ol.LocalVolSurface and create_sample_iv_surface is ol.create_sample_iv_surface
    finally:
        compat.uninstall()
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
