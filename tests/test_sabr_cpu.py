"""CPU checks of the SABR family (include/olmc_sabr.h, optionslab_amd/sabr.py).

  golden   the package's implied_vol and price against tests/golden/sabr.json, recorded from the reference, at 1e-12 relative on every
           row: the expired, at-the-money, small-z and general branches, beta in {0, 0.5, 0.7, 1}, calls and puts.
  fits     calibrate_sabr against the reference's four results at 1e-6 relative: the same objective through the same L-BFGS-B, so the
           iterates differ by the rounding of the objective alone.  Measured here: 0 on every parameter of every case (the two
           implementations round alike), so the bar stays at its start of 1e-6.  The alpha = 2.0 bound case matches exactly.
  ABI      olmc_sabr.h's declarations = the library's olsb_* exports = _hip.SABR_PROTOTYPES; the header is C99; every refusal answers
           OLMC_ERR_ARG with its exact message, in the header's order, before any device is touched.
  Python   the refusals raise before the library is loaded; the reference's import lines resolve under compat.
  oracle   tests/sabr_oracle.py with the reference Box-Muller: nu = 0, beta = 1 is a GBM recursion; the mirror of the mirror is the path;
           the conditions tests/test_gpu_sabr.py asserts of the device's draws (no pre-clamp G within 1e-7 of 0, at least 2 % of 4133
           paths absorbed at 64 steps under each absorbing model, no live state within 1e-9 of a barrier level in log space) hold for
           its cases here too.
"""
import ctypes as C
import inspect
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import path_draw_oracle as pdo
from tests import sabr_oracle as so
from tests.abi_support import assert_header_matches, library, no_library, refused  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc_sabr.h")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "sabr.json")))


# ------------------------------------------------------------------------------------------------------------ golden ----
def test_hagan_matches_the_reference_on_every_branch():
    branches = {}
    worst = 0.0
    with np.errstate(all="ignore"):                          # nu = 0: 0 / 0 is formed before the small-z branch is taken, as in the reference
        for row in GOLDEN["grid"]:
            model = ol.SABRModel(row["alpha"], row["beta"], row["rho"], row["nu"])
            got = (model.implied_vol(row["F"], row["K"], row["T"]), model.price(row["F"], row["K"], row["T"], row["r"], "call"),
                   model.price(row["F"], row["K"], row["T"], row["r"], "put"))
            for g, w in zip(got, (row["implied_vol"], row["call"], row["put"])):
                assert abs(g - w) <= 1e-12 * abs(w), row
                if w:
                    worst = max(worst, abs(g - w) / abs(w))
            branches[row["branch"]] = branches.get(row["branch"], 0) + 1
    print("DEVIATION " + json.dumps(dict(test="hagan-vs-reference", worst_rel=worst, rows=branches)))
    assert set(branches) == {"expired", "atm", "small-z", "general"} and min(branches.values()) >= 48
    assert {row["beta"] for row in GOLDEN["grid"]} == {0.0, 0.5, 0.7, 1.0}


def test_smile_and_black_price_by_hand():
    model = ol.SABRModel(0.25, 1.0, -0.4, 0.5)
    ks = np.array([80.0, 100.0, 125.0])
    assert np.array_equal(model.smile(100.0, 1.0, ks), np.array([model.implied_vol(100.0, k, 1.0) for k in ks]))
    assert model.implied_vol(100.0, 90.0, 0.0) == 0.25 and model.price(100.0, 90.0, 0.0, 0.03, "call") == 10.0
    assert ol.SABRModel._black_price(100.0, 90.0, 0.0, 0.03, 0.2, "put") == 0.0
    call, put = (ol.SABRModel._black_price(100.0, 110.0, 2.0, 0.03, 0.3, kind) for kind in ("call", "put"))
    assert call - put == pytest.approx(np.exp(-0.06) * (100.0 - 110.0), rel=1e-13)            # parity on the forward


@pytest.mark.parametrize("case", GOLDEN["calibrations"], ids=lambda c: c["name"])
def test_calibration_matches_the_reference(case):
    fit = ol.calibrate_sabr(case["F"], case["T"], np.array(case["strikes"]), np.array(case["market_vols"]), beta=case["truth"][1])
    got, want = [fit.alpha, fit.beta, fit.rho, fit.nu], case["fitted"]
    print("DEVIATION " + json.dumps(dict(test="calibration", case=case["name"], rel=[abs(g - w) / abs(w) for g, w in zip(got, want)])))
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-6 * abs(w), (case["name"], got, want)
    if case["name"] == "alpha-bound":
        assert fit.alpha == want[0] == 2.0 and case["truth"][0] == 2.5                        # the reference's cap, kept
    else:
        assert np.allclose(got, case["truth"], rtol=0, atol=1e-4)                             # noise-free smiles: the truth comes back


# --------------------------------------------------------------------------------------------------------------- ABI ----
def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "olsb_", _hip.SABR_PROTOTYPES, ["olsb_paths", "olsb_price", "olsb_surface_prices"])
    assert not set(_hip.SABR_PROTOTYPES) & set(_hip.PROTOTYPES)
    assert _hip.STREAM_SABR == 0x53414252 == int.from_bytes(b"SABR", "big") == so.TAG_SABR and _hip.SABR_EUROPEAN == 8


def test_header_is_c99_and_the_struct_is_four_doubles(tmp_path):
    assert C.sizeof(_hip.SabrModel) == 32 and [f for f, _ in _hip.SabrModel._fields_] == ["alpha", "beta", "rho", "nu"]
    from optionslab_amd.build import _hipcc

    cc = shutil.which("gcc") or shutil.which("cc")
    compiler = [cc] if cc else [_hipcc(), "-x", "c"]
    src = tmp_path / "use_header.c"
    src.write_text('#include "olmc_sabr.h"\n'
                   "typedef char model_is_32_bytes[sizeof(olsb_model) == 32 ? 1 : -1];\n"
                   "typedef char european_is_8[OLSB_EUROPEAN == 8 && OLMC_PATH_ASIAN_GEOMETRIC == 7 && OLMC_STREAM_SABR == 0x53414252u ? 1 : -1];\n"
                   "int use(const olsb_model* m, olmc_stats* out) { return olsb_price(100, 100, 1, 0.03, 1, m, OLSB_EUROPEAN, 0, 0, 1000, 8, 1, 0, out); }\n")
    subprocess.run([*compiler, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use_header.o")], check=True)


def entry_calls(library, m, *, F=100.0, payoff=8, barrier=0.0, offset=0, n=100, steps=4, k=2, out=True, cells=True):
    """The three entry points on the model pointer m, as thunks that give the return code."""
    st = _hip.Stats()
    sts = (_hip.Stats * 16)()
    strikes, cell_steps = (C.c_double * 16)(*([100.0] * 16)), (C.c_int32 * 16)(*([1] * 16))
    fwd, vol = (C.c_double * 8)(), (C.c_double * 8)()
    return {
        "olsb_price": lambda: library.olsb_price(F, 100.0, 1.0, 0.03, 1, m, payoff, barrier, offset, n, steps, 7, 0, C.byref(st) if out else None),
        "olsb_paths": lambda: library.olsb_paths(F, 1.0, m, n, steps, 7, 0, 1, fwd if out else None, vol),
        "olsb_surface_prices": lambda: library.olsb_surface_prices(F, 1.0, 0.03, 1, m, strikes if cells else None, cell_steps, k, offset, n, steps, 7, 0,
                                                                   sts if out else None),
    }


# in the header's order: each model carries this fault and every later one, so the message says which check came first
BAD_MODELS = [
    ((0.0, 2.0, 3.0, -1.0), "alpha must be positive"), ((-0.1, 0.5, 0.0, 0.4), "alpha must be positive"),
    ((0.2, -0.1, 3.0, -1.0), "beta must be in [0, 1]"), ((0.2, 1.5, 0.0, 0.4), "beta must be in [0, 1]"), ((0.2, float("nan"), 0.0, 0.4), "beta must be in [0, 1]"),
    ((0.2, 0.5, -1.5, -1.0), "rho must be in [-1, 1]"), ((0.2, 0.5, 1.01, 0.4), "rho must be in [-1, 1]"), ((0.2, 0.5, float("nan"), 0.4), "rho must be in [-1, 1]"),
    ((0.2, 0.5, 0.0, -0.4), "nu must be non-negative"),
]


@pytest.mark.parametrize("entry", sorted(_hip.SABR_PROTOTYPES))
def test_every_refusal_answers_its_message_before_any_device_work(library, entry):
    """rc 1 (OLMC_ERR_ARG) and the exact words, on a machine with or without a device: none of these calls initialises one."""
    good = _hip.sabr_model(0.25, 0.5, -0.3, 0.4)
    call = lambda m=C.byref(good), **kw: entry_calls(library, m, **kw)[entry]()
    refused(library, call(m=None), "null pointer")
    refused(library, call(out=False), "null pointer")
    if entry == "olsb_surface_prices":
        refused(library, call(cells=False), "null pointer")
    for params, message in BAD_MODELS:
        bad = _hip.sabr_model(*params)
        refused(library, call(m=C.byref(bad), F=-1.0, n=0, payoff=9), message)          # the model before F, the payoff and the counts
    refused(library, call(F=0.0, n=0, payoff=9), "F must be positive")
    refused(library, call(F=-3.0), "F must be positive")
    for edge in ((1e-300, 0.0, -1.0, 0.0), (0.2, 1.0, 1.0, 0.0)):                          # the closed ends of every range are served
        ok = _hip.sabr_model(*edge)
        refused(library, call(m=C.byref(ok), n=0), "n_paths must be >= 1")
    refused(library, call(n=0), "n_paths must be >= 1")
    refused(library, call(steps=0), "n_steps must be >= 1")
    refused(library, call(n=0, steps=0), "n_paths must be >= 1")
    if entry != "olsb_paths":
        refused(library, call(offset=-1), "path_offset must be >= 0")
    if entry == "olsb_price":
        refused(library, call(payoff=-1), "bad payoff")
        refused(library, call(payoff=9), "bad payoff")
        for kind in range(4):
            refused(library, call(payoff=kind, barrier=0.0), "Barrier must be positive")
            refused(library, call(payoff=kind, barrier=-5.0), "Barrier must be positive")
        refused(library, call(payoff=9, steps=0), "bad payoff")                          # as ollv_price: the payoff before the range
        refused(library, call(payoff=0, barrier=0.0, n=0), "Barrier must be positive")
    if entry == "olsb_surface_prices":
        refused(library, call(k=0), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        refused(library, call(k=17), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        refused(library, call(k=17, steps=0), "n_steps must be >= 1")
        sts = (_hip.Stats * 2)()
        strikes, steps = (C.c_double * 2)(100.0, 100.0), (C.c_int32 * 2)(1, 5)
        refused(library, library.olsb_surface_prices(100.0, 1.0, 0.03, 1, C.byref(good), strikes, steps, 2, 0, 100, 4, 7, 0, sts),
                "a cell's step must be in [1, n_steps]")
    if entry == "olsb_paths":
        refused(library, call(n=1 << 33, steps=1), "path matrices would exceed 64 GB")
        refused(library, call(n=1 << 33, steps=0), "n_steps must be >= 1")


# ------------------------------------------------------------------------------------------------------------ Python ----
def test_python_surface_of_the_model():
    for name in ("SABRModel", "calibrate_sabr", "SABRAdapter", "SABRMCAdapter", "greeks_sabr"):
        assert name in ol.__all__ and getattr(ol, name) is getattr(ol.sabr, name)
    assert list(inspect.signature(ol.SABRModel).parameters) == ["alpha", "beta", "rho", "nu"]
    assert list(inspect.signature(ol.SABRModel.price).parameters) == ["self", "F", "K", "T", "r", "option_type"]
    assert list(inspect.signature(ol.calibrate_sabr).parameters) == ["F", "T", "strikes", "market_vols", "beta", "initial_guess"]
    for name in ("price_monte_carlo", "price_asian", "price_barrier", "price_lookback", "price_surface"):
        want = ["F" if p == "S" else p for p in inspect.signature(getattr(ol.DupireLocalVol, name)).parameters if p != "q"]
        assert list(inspect.signature(getattr(ol.SABRModel, name)).parameters) == want, name
        for p, v in inspect.signature(getattr(ol.DupireLocalVol, name)).parameters.items():
            if p not in ("S", "q"):
                assert inspect.signature(getattr(ol.SABRModel, name)).parameters[p].default == v.default, (name, p)
    assert list(inspect.signature(ol.SABRModel.simulate_paths).parameters) == ["self", "F", "T", "n_paths", "n_steps", "seed", "mirror"]
    assert list(inspect.signature(ol.SABRModel.smile_monte_carlo).parameters)[:4] == ["self", "F", "T", "strikes"]
    assert ol.SABRModel(0.2, 0.5, -0.3, 0.4) == ol.SABRModel(0.2, 0.5, -0.3, 0.4)


@pytest.mark.parametrize("params,message", [((0.0, 0.5, 0.0, 0.4), "alpha must be positive"), ((0.2, 1.1, 0.0, 0.4), "beta must be in [0, 1]"),
                                            ((0.2, -0.1, 0.0, 0.4), "beta must be in [0, 1]"), ((0.2, 0.5, -1.1, 0.4), "rho must be in [-1, 1]"),
                                            ((0.2, 0.5, 0.0, -0.1), "nu must be non-negative")])
def test_the_model_refuses_with_the_reference_s_messages(params, message):
    with pytest.raises(ValueError, match=message.replace("[", r"\[").replace("]", r"\]")):
        ol.SABRModel(*params)


def test_python_refusals_come_before_the_library_is_loaded(no_library):
    model = ol.SABRModel(0.25, 0.5, -0.3, 0.4)
    refusals = [
        lambda: model.price_monte_carlo(0.0, 100, 1.0, 0.03), lambda: model.price_monte_carlo(-1.0, 100, 1.0, 0.03),
        lambda: model.price_monte_carlo(float("nan"), 100, 1.0, 0.03),
        lambda: model.price_monte_carlo(100, 100, 1.0, 0.03, n_paths=0), lambda: model.price_monte_carlo(100, 100, 1.0, 0.03, n_steps=0),
        lambda: model.simulate_paths(100, 1.0, n_paths=0), lambda: model.simulate_paths(0.0, 1.0),
        lambda: model.price_barrier(100, 100, 1.0, 0.03, 0.0), lambda: model.price_barrier(100, 100, 1.0, 0.03, -5.0),
        lambda: model.price_asian(100, 100, 1.0, 0.03, avg_type="harmonic"), lambda: model.price_lookback(100, 100, 1.0, 0.03, lookback_type="partial"),
        lambda: model.price_surface(100, [100.0], [0.3, 1.0], 0.03, n_steps=4), lambda: model.price_surface(100, [], [1.0], 0.03),
        lambda: model.price_surface(0.0, [100.0], [1.0], 0.03), lambda: model.smile_monte_carlo(100, 1.0, []),
        lambda: model.smile_monte_carlo(0.0, 1.0, [100.0]), lambda: model.smile_monte_carlo(100, 1.0, [100.0], n_paths=0),
    ]
    for refusal in refusals:
        with pytest.raises(ValueError):
            refusal()
    with pytest.raises(AssertionError, match="the library was loaded"):                       # the fixture does bite: a good call reaches for it
        model.price_monte_carlo(100, 100, 1.0, 0.03, n_paths=10, n_steps=2, seed=1)


def test_adapters_and_greeks():
    model = ol.SABRModel(0.2, 1.0, -0.3, 0.4)
    S, K, T, r, q = 100.0, 105.0, 1.0, 0.03, 0.01
    forward = S * np.exp((r - q) * T)
    assert ol.SABRAdapter(model).price(S, K, T, r, 0.9, "put", q) == model.price(forward, K, T, r, "put")
    assert isinstance(ol.SABRAdapter(model), ol.PricerProtocol) and isinstance(ol.SABRMCAdapter(model), ol.PricerProtocol)
    greeks = ol.greeks_sabr(model, S, K, T, r, "call", q)
    assert list(greeks) == ["price", "delta", "gamma", "vega", "theta", "rho", "vanna", "charm", "vomma"]
    assert greeks["price"] == model.price(forward, K, T, r, "call") and 0.0 < greeks["delta"] < 1.0 and greeks["gamma"] > 0.0
    assert greeks["vega"] == 0.0 and greeks["vomma"] == 0.0                                    # sigma is ignored
    want = ol.compute_greeks_unified(ol.SABRAdapter(model), S, K, T, r, 0.2, "call", q)
    assert greeks == want
    mc = ol.SABRMCAdapter(model, 1 << 14, 16, 5, True)
    assert (mc.n_paths, mc.n_steps, mc.seed, mc.antithetic) == (1 << 14, 16, 5, True)


def test_compat_serves_the_reference_s_import_lines():
    import optionslab_amd.compat as compat

    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    try:
        compat.install()
        from src.greeks import SABRAdapter, greeks_sabr
        from src.greeks.unified_greeks import SABRAdapter as adapter_by_module
        from src.pricing_models import HestonPricer, MertonJumpDiffusion, SABRModel, calibrate_sabr
        from src.pricing_models.sabr import SABRModel as model_by_module
        assert SABRModel is model_by_module is ol.SABRModel and calibrate_sabr is ol.calibrate_sabr
        assert SABRAdapter is adapter_by_module is ol.SABRAdapter and greeks_sabr is ol.greeks_sabr
        assert HestonPricer is ol.HestonPricer and MertonJumpDiffusion is ol.MertonJumpDiffusion
    finally:
        compat.uninstall()
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ------------------------------------------------------------------------------------------------------------ oracle ----
REF = pdo.reference_box_muller


def test_oracle_draws_are_the_heston_layout_under_the_sabr_tag():
    z1, z2 = so.draws(so.SEED, 5, 3, 5, REF)
    raw = pdo.draws(so.SEED, 5, 3, 3, so.TAG_SABR, REF)[1]
    assert z1.shape == z2.shape == (3, 5)
    assert np.array_equal(z1[:, 2], raw[:, 1, 0]) and np.array_equal(z2[:, 2], raw[:, 1, 1])   # step 2 = block 1, (cos, sin)(x0, x1)
    assert np.array_equal(z1[:, 3], raw[:, 1, 2]) and np.array_equal(z2[:, 3], raw[:, 1, 3])   # step 3 = block 1, (cos, sin)(x2, x3)
    assert not np.array_equal(pdo.draws(so.SEED, 5, 3, 3, pdo.TAG_HESTON, REF)[0], pdo.draws(so.SEED, 5, 3, 3, so.TAG_SABR, REF)[0])


def test_oracle_without_vol_of_vol_and_beta_one_is_a_gbm_recursion():
    for n in (1, 5, 64):
        z1, z2 = so.draws(so.SEED, 0, 257, n, REF)
        forward, vol, closest = so.paths(so.F0, so.T, (0.25, 1.0, -0.4, 0.0), n, z1, z2)
        want = so.gbm_paths(so.F0, so.T, 0.25, n, z1)
        assert np.all(vol == 0.25) and closest == np.inf
        assert float(np.max(np.abs(forward / want - 1))) <= 1e-15 * (n + 2)


def test_oracle_mirror_of_the_mirror_is_the_path():
    for name, model in so.MODELS.items():
        z1, z2 = so.draws(so.SEED, 0, 100, 13, REF)
        plain = so.paths(so.F0, so.T, model, 13, z1, z2)
        mirror = so.paths(so.F0, so.T, model, 13, z1, z2, mirror=True)
        back = so.paths(so.F0, so.T, model, 13, -z1, -z2, mirror=True)
        assert np.array_equal(back[0], plain[0]) and np.array_equal(back[1], plain[1]), name
        assert not np.array_equal(mirror[0][:, 1:], plain[0][:, 1:])
        assert np.all(plain[0][:, 0] == so.F0) and np.all(plain[1][:, 0] == model[0])


def test_oracle_absorbed_paths_stay_at_zero_and_pay_as_zero():
    z1, z2 = so.draws(so.SEED, 0, 4133, 64, REF)
    forward = so.paths(so.F0, so.T, so.MODELS["normal-absorbing"], 64, z1, z2)[0].astype(np.float64)
    dead = forward[:, -1] == 0
    first = np.argmax(forward == 0, axis=1)
    assert dead.any() and np.all(forward[forward[:, -1] > 0] > 0)
    for row, at in zip(forward[dead][:50], first[dead][:50]):
        assert np.all(row[at:] == 0) and np.all(row[:at] > 0)
    assert np.all(so.payoffs(forward[dead], 7, True, 50.0) == 0) and np.all(so.payoffs(forward[dead], 3, False, 100.0, so.DOWN) == 100.0)
    assert np.all(so.payoffs(forward[dead], 2, False, 100.0, so.DOWN) == 0) and np.all(so.payoffs(forward[dead], 5, False, 100.0) == 100.0)


@pytest.mark.parametrize("name", sorted(so.MODELS))
def test_the_gpu_module_s_conditions_hold_with_the_reference_box_muller(name):
    """No pre-clamp G within 1e-7 of 0, no live state within 1e-9 of a level in log space, at every shape of the GPU module; each
    absorbing model absorbs at least 2 % of 4133 paths at 64 steps, plain and mirror."""
    model = so.MODELS[name]
    for N in so.PATHS:
        for n in so.STEPS:
            z1, z2 = so.draws(so.SEED, 0, N, n, REF)
            for mirror in (False, True):
                forward, _vol, closest = so.paths(so.F0, so.T, model, n, z1, z2, mirror)
                assert closest > 1e-7, (name, N, n, mirror, closest)
                assert so.level_clearance(forward.astype(np.float64)) > 1e-9, (name, N, n, mirror)
                if name in so.ABSORBING and (N, n) == (4133, 64):
                    absorbed = int(np.sum(forward[:, -1] == 0))
                    print("DEVIATION " + json.dumps(dict(test="absorbed", model=name, mirror=mirror, paths=absorbed, closest_g=closest)))
                    assert absorbed >= 0.02 * N
                if name not in so.ABSORBING and model[1] == 1.0:
                    assert np.all(forward > 0)
