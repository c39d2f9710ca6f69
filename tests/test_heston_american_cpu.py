"""CPU checks of the American option under Heston (include/olha.h, HestonPricer.price_american).  No GPU: the library is loaded, never a
device.

  ABI        the header's declarations = the library's olha_* exports = _hip.HA_PROTOTYPES; the header is plain C.
  oracle     tests/heston_american_oracle.py without its y monomials is oracle/numpy_reference.py's american_from_paths; its exercise
             decisions do not change when (S / K, v / theta) are replaced by the library's standardised regressors and lstsq by the
             normal equations (the device's parametrisation and solve), on the prototype's five models and degrees 1 .. 3.
  scales     olha_regressor_scales: finite and positive for t -> 0, sigma_v = 0 and v0 = theta; the closed forms themselves.
  refusals   every message of the C ABI, before any device work; price_american's ValueErrors and its T <= 0 early-out before the
             library is loaded.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from optionslab_amd import _hip
from oracle import numpy_reference as orc
from tests import heston_american_cases as hc
from tests import heston_american_oracle as hao
from tests.abi_support import assert_header_matches, library, no_library, refused
from tests.gpu_support import heston_pricer
from tests.test_jump_payoffs_cpu import c_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olha.h")
NAMES = ["olha_american_lsm", "olha_american_lsm_qmc", "olha_regressor_scales"]
S, K, T, R = 100.0, 100.0, 1.0, 0.05


# --------------------------------------------------------------------------------------------------------- the ABI ----
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_header.c"
    src.write_text('#include "olha.h"\n'
                   "int use(const uint32_t* sv, const uint32_t* shift, double* a, olmc_stats* out) {\n"
                   "    return olha_american_lsm(100, 100, 1, 0.05, 0, 0, 2, 0.04, 0.3, -0.7, 0.04, OLHA_EULER, OLHA_BASIS_SPOT_VARIANCE, 2, 1000, 8, 1, out)\n"
                   "        + olha_american_lsm_qmc(100, 100, 1, 0.05, 0, 0, 2, 0.04, 0.3, -0.7, 0.04, OLHA_QE, OLHA_BASIS_SPOT, 3, OLMC_QMC_SEQUENTIAL, 1000, sv,\n"
                   "                                shift, 16, 30, out)\n"
                   "        + olha_regressor_scales(100, 100, 1, 0.05, 0, 0, 2, 0.04, 0.3, 0.04, 8, a, a + 9, a + 18, a + 27); }\n")
    subprocess.run([*c_compiler(), "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "olha_", _hip.HA_PROTOTYPES, NAMES)
    for other in (_hip.PROTOTYPES, _hip.LV_PROTOTYPES, _hip.LVQ_PROTOTYPES, _hip.JD_PROTOTYPES, _hip.JS_PROTOTYPES):
        assert not any(name.startswith("olha_") for name in other)
    for name in ("heston_american_lsm", "heston_american_lsm_qmc", "heston_american_scales"):
        assert callable(getattr(_hip, name))
    assert (_hip.HA_BASIS_SPOT_VARIANCE, _hip.HA_BASIS_SPOT) == (0, 1)


# ------------------------------------------------------------------------------------------------------ the oracle ----
@pytest.mark.parametrize("typ,q,degree", [("put", 0.0, 1), ("put", 0.0, 3), ("call", 0.06, 2)])
def test_without_the_variance_monomials_the_oracle_is_the_one_factor_reference(typ, q, degree):
    spot, var = orc.heston_simulate_paths(S, T, R, q, *hao.MODELS["usual"], 8000, 20, seed=5)
    want, x = orc.american_from_paths(spot, K, T, R, typ, degree, return_payoffs=True)
    price, cf, margin = hao.american_from_state(spot, var, K, T, R, 0.04, typ, degree, with_variance=False)
    assert margin > 1e-9                                  # no decision within rounding of its threshold: the two fits decide alike
    assert price == pytest.approx(want, rel=1e-12) and np.allclose(cf, x, rtol=1e-12, atol=0.0)


RUNS = [("usual", 30_000, 50), ("calm", 20_000, 25), ("high-vol-of-vol", 20_000, 50), ("extreme", 10_000, 12), ("fast-reversion", 30_000, 33)]


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("name,n_paths,n_steps", RUNS)
def test_the_oracle_decides_alike_in_the_device_s_parametrisation(library, name, n_paths, n_steps, degree):
    """lstsq on the monomials of (S / K, v / theta) against the normal equations in the library's standardised regressors: zero
    differing exercise decisions, hence the same cash flows."""
    model = hao.MODELS[name]
    kappa, theta, sigma_v, _rho, v0 = model
    spot, var = orc.heston_simulate_paths(S, T, R, 0.0, *model, n_paths, n_steps, seed=11)
    cx, wx, cy, wy = _hip.heston_american_scales(S, K, T, R, 0.0, False, kappa, theta, sigma_v, v0, n_steps)

    def standardised(t, s, v):
        return (s / K - cx[t]) / wx[t], (v - cy[t]) / wy[t]

    price, cf, margin, decisions = hao.american_from_state(spot, var, K, T, R, theta, "put", degree, return_decisions=True)
    price_ne, cf_ne, _margin, decisions_ne = hao.american_from_state(spot, var, K, T, R, theta, "put", degree, regressors=standardised,
                                                                     fit=hao.normal_equations_fit, return_decisions=True)
    print(name, degree, "price", price, "margin", margin, "decisions", int(decisions.sum()))
    assert decisions.any() and np.array_equal(decisions, decisions_ne)
    assert np.array_equal(cf, cf_ne) and price == price_ne


def test_a_higher_degree_in_the_state_prices_higher_than_the_spot_alone():
    """What the feature is for: on one path set the (S, v) fit's price rises with the degree and lies above the one-factor fit's."""
    model = hao.MODELS["usual"]
    spot, var = orc.heston_simulate_paths(S, T, R, 0.0, *model, 30_000, 50, seed=11)
    prices = [hao.american_from_state(spot, var, K, T, R, model[1], "put", d)[0] for d in (1, 2, 3)]
    spot_only = hao.american_from_state(spot, var, K, T, R, model[1], "put", 3, with_variance=False)[0]
    assert prices[0] < prices[1] < prices[2] and spot_only < prices[1]


# ------------------------------------------------------------------------------------------------------ the scales ----
def test_the_scale_pairs_are_finite_and_positive_at_the_edges(library):
    cases = [
        (hao.MODELS["usual"], 1e-9, 50),                                   # t -> 0
        (hao.MODELS["usual"], 1.0, 4096),
        ((2.0, 0.04, 0.0, -0.7, 0.04), 1.0, 50),                           # sigma_v = 0 and v0 = theta: v_t is theta itself
        ((2.0, 0.04, 0.0, -0.7, 0.09), 1.0, 50),                           # sigma_v = 0: v_t is deterministic
        ((0.0, 0.04, 0.3, -0.7, 0.04), 1.0, 12),                           # kappa = 0
        (hao.MODELS["extreme"], 5.0, 12),
    ]
    for (kappa, theta, sigma_v, _rho, v0), T_, n in cases:
        for is_call, strike in ((False, 100.0), (True, 100.0), (False, 40.0), (True, 250.0)):
            cx, wx, cy, wy = _hip.heston_american_scales(S, strike, T_, R, 0.01, is_call, kappa, theta, sigma_v, v0, n)
            for a in (cx, wx, cy, wy):
                assert a.shape == (n + 1,) and np.all(np.isfinite(a))
            assert np.all(wx > 0) and np.all(wy > 0) and np.all(cx > 0) and np.all(cy >= 0)
            assert (cx[0], wx[0], cy[0], wy[0]) == (1.0, 1.0, 0.0, 1.0) == (cx[n], wx[n], cy[n], wy[n])      # dates no regression reads
    cx, wx, cy, wy = _hip.heston_american_scales(S, K, T, R, 0.0, False, 2.0, 0.04, 0.0, 0.04, 50)
    assert np.all(cy[1:50] == 0.04) and np.allclose(wy[1:50], 1e-6 * 0.04, rtol=1e-14, atol=0.0)     # y = (v - theta) / width is exactly 0 on v = theta


def test_the_scale_pairs_are_the_closed_forms(library):
    kappa, theta, sigma_v, _rho, v0 = hao.MODELS["high-vol-of-vol"]
    n = 25
    cx, wx, cy, wy = _hip.heston_american_scales(S, K, T, R, 0.02, False, kappa, theta, sigma_v, v0, n)
    phi = lambda u: 0.5 * math.erfc(-u / math.sqrt(2.0))
    for t in (1, 7, 24):
        tau = T * t / n
        e = math.exp(-kappa * tau)
        mean = theta + (v0 - theta) * e
        var = v0 * sigma_v**2 * e * (1 - e) / kappa + theta * sigma_v**2 * (1 - e) ** 2 / (2 * kappa)
        assert cy[t] == pytest.approx(mean, rel=1e-13) and wy[t] == pytest.approx(math.sqrt(var), rel=1e-12)
        sig2 = theta + (v0 - theta) * (1 - e) / (kappa * tau)              # the expected average variance over [0, tau]
        m, s, a = math.log(S) + (R - 0.02 - 0.5 * sig2) * tau, math.sqrt(sig2 * tau), math.log(K)
        p0, m1, m2 = phi(-(m - a) / s), math.exp(m + 0.5 * s * s) * phi(-(m + s * s - a) / s), math.exp(2 * m + 2 * s * s) * phi(-(m + 2 * s * s - a) / s)
        assert cx[t] == pytest.approx(m1 / p0 / K, rel=1e-12)
        assert wx[t] == pytest.approx(math.sqrt(m2 / p0 - (m1 / p0) ** 2) / K, rel=1e-9)


# ---------------------------------------------------------------------------------------------------- the refusals ----
@pytest.mark.parametrize("name,args,message", hc.REFUSALS, ids=hc.REFUSAL_IDS)
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    refused(library, getattr(library, name)(*args()), message)


@pytest.mark.parametrize("kwargs,message", [
    (dict(option_type="straddle"), "option_type must be 'call' or 'put'"),
    (dict(basis="variance"), "basis must be 'spot_variance' or 'spot'"),
    (dict(scheme="milstein"), "scheme must be 'euler' or 'qe'"),
    (dict(poly_degree=0), "poly_degree must be in [1, 3] for basis='spot_variance'"),
    (dict(poly_degree=4), "poly_degree must be in [1, 3] for basis='spot_variance'"),
    (dict(poly_degree=5, basis="spot"), "poly_degree must be in [1, 4] for basis='spot'"),
    (dict(n_paths=0), "n_paths and n_steps must be >= 1"),
    (dict(n_steps=0), "n_paths and n_steps must be >= 1"),
    (dict(scheme="qe", method="qmc"), "scheme='qe' with method='qmc' takes path_construction='sequential'"),
    (dict(method="sobol"), "method must be 'pseudo' or 'qmc'"),
    (dict(method="qmc", path_construction="zigzag"), "path_construction must be 'bridge' or 'sequential'"),
    (dict(method="qmc", n_steps=2000), "path_construction='bridge' takes at most 1024 steps"),
])
def test_price_american_refuses_before_the_library_is_loaded(no_library, kwargs, message):
    with pytest.raises(ValueError, match=message.replace("[", r"\[").replace("]", r"\]")):
        heston_pricer(hao.MODELS["usual"]).price_american(S, K, T, R, **kwargs)


def test_an_expired_option_is_its_intrinsic_value_without_simulating(no_library):
    p = heston_pricer(hao.MODELS["usual"])
    assert p.price_american(90.0, 100.0, 0.0, R) == 10.0 and p.price_american(90.0, 100.0, -1.0, R, option_type="call") == 0.0
    assert p.price_american(110.0, 100.0, 0.0, R, option_type="call", return_error=True, method="qmc", scheme="qe", path_construction="sequential") == (10.0, 0.0)
    with pytest.raises(ValueError):
        p.price_american(90.0, 100.0, 0.0, R, n_paths=0)               # the refusals come first


def test_price_american_has_the_documented_signature():
    import inspect

    sig = inspect.signature(heston_pricer(hao.MODELS["usual"]).price_american)
    assert [(n, p.default) for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty] == [
        ("q", 0.0), ("option_type", "put"), ("n_paths", 50000), ("n_steps", 50), ("poly_degree", 2), ("seed", None), ("return_error", False),
        ("basis", "spot_variance"), ("scheme", "euler"), ("method", "pseudo"), ("path_construction", "bridge")]
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["basis", "scheme", "method", "path_construction"]
