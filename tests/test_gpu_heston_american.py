"""The American option under Heston (include/olha.h, HestonPricer.price_american) on the device, tied per seed to the NumPy oracle
(tests/heston_american_oracle.py: lstsq on the monomials of (S / K, v / theta)) applied to the device's own path matrices.

The tie is the project's AMERICAN_TIE: n ==, sum and price at 1e-9, sumsq at 2e-9; one flipped exercise decision moves a price by about
1e-5.  Device and oracle fit the same polynomial space in other coordinates and by another solver, so their continuation values differ
by rounding, and a path whose intrinsic value lies that close to its continuation value may decide differently.  GUARD keeps the cases
away from such paths: every tied case asserts that the oracle's smallest |intrinsic - continuation| is above it.
GUARD = 3e-7: the largest |continuation by the normal equations in standardised regressors - continuation by lstsq| over the CPU
prototype's 15 runs (NumPy Euler paths of the five models of heston_american_oracle.MODELS, 10,000 .. 30,000 paths x 12 .. 50 dates,
degrees 1 .. 3, the cash flows of the lstsq run at every date) is 2.95e-9 (sigma_v = 1, rho = -0.9, degree 3; moment matrix condition
4.2e5), times 100.  A case whose margin falls under the guard is given another seed when this file is written; with seed 7 none of
the cases below does (the smallest margin is 1.5e-6).
"""
import functools
import math

import numpy as np
import pytest

from optionslab_amd import _hip
from optionslab_amd.monte_carlo import sobol_tables
from oracle import numpy_reference as orc
from tests import heston_american_cases as hc
from tests import heston_american_oracle as hao
from tests.abi_support import library, refused
from tests.gpu_support import device_fixture, heston_pricer
from tests.test_gpu_american_qmc import AMERICAN_TIE, AMERICAN_TIE_DEGREE_4, assert_tied

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]
_device = device_fixture()

GUARD = 3e-7
T, R = 1.0, 0.05
PUT, CALL = (100.0, 100.0, 0.0, False), (100.0, 95.0, 0.06, True)                # S K q is_call
USUAL, HIGH, EXTREME = hao.MODELS["usual"], hao.MODELS["high-vol-of-vol"], hao.MODELS["extreme"]
# how the paths are drawn: (Sobol construction or None for Philox, quadratic-exponential scheme)
EULER, QE, SOBOL, SOBOL_BRIDGE, SOBOL_QE = (None, False), (None, True), ("sequential", False), ("bridge", False), ("sequential", True)


def matrices(draw, model, S, q, n_paths, n_steps, seed):
    """The device's own (n_paths, n_steps + 1) spot and variance matrices of the draw."""
    construction, qe = draw
    if construction is None:
        paths = _hip.heston_qe_paths if qe else _hip.heston_paths
        return paths(S, T, R, q, *model, n_paths, n_steps, seed, path_major=True)
    sv, shift = sobol_tables(2 * n_steps, seed, n_paths)
    paths = _hip.heston_qe_qmc_paths if qe else _hip.heston_qmc_paths
    return paths(S, T, R, q, *model, n_paths, sv, shift, construction == "bridge", path_major=True)


def price(draw, model, S, K, q, call, n_paths, n_steps, seed, degree, spot_basis=False):
    construction, qe = draw
    if construction is None:
        return _hip.heston_american_lsm(S, K, T, R, q, call, *model, n_paths, n_steps, seed, degree, spot_basis, qe)
    sv, shift = sobol_tables(2 * n_steps, seed, n_paths)
    return _hip.heston_american_lsm_qmc(S, K, T, R, q, call, *model, n_paths, sv, shift, construction == "bridge", degree, spot_basis, qe)


def tie(draw, model, contract, n_paths, n_steps, degree, seed):
    S, K, q, call = contract
    st = price(draw, model, S, K, q, call, n_paths, n_steps, seed, degree)
    spot, var = matrices(draw, model, S, q, n_paths, n_steps, seed)
    want, x, margin = hao.american_from_state(spot, var, K, T, R, model[1], "call" if call else "put", degree)
    print("price", st.price, "oracle", want, "margin", margin)
    assert margin > GUARD
    assert_tied(st, want, x, AMERICAN_TIE)
    return st


# ------------------------------------------------------------------------------------------------- 1. the tie ----
LARGE, MEDIUM, TWO, ONE, RAGGED = (20_001, 50), (10_007, 13), (4_097, 2), (5_000, 1), (300_001, 3)
CASES = [
    (EULER, USUAL, PUT, LARGE, 2, 7), (EULER, HIGH, PUT, LARGE, 3, 7), (EULER, EXTREME, PUT, MEDIUM, 1, 7), (EULER, USUAL, CALL, MEDIUM, 2, 7),
    (EULER, EXTREME, PUT, TWO, 3, 7), (EULER, USUAL, PUT, ONE, 2, 7), (EULER, HIGH, PUT, RAGGED, 2, 7),
    (QE, USUAL, PUT, LARGE, 2, 7), (QE, EXTREME, PUT, MEDIUM, 3, 7), (QE, HIGH, CALL, TWO, 1, 7), (QE, USUAL, PUT, RAGGED, 1, 7),
    (SOBOL, USUAL, PUT, MEDIUM, 2, 7), (SOBOL, HIGH, PUT, LARGE, 1, 7), (SOBOL, EXTREME, CALL, TWO, 3, 7), (SOBOL, USUAL, PUT, RAGGED, 3, 7),
    (SOBOL_BRIDGE, USUAL, PUT, LARGE, 3, 7), (SOBOL_BRIDGE, EXTREME, CALL, MEDIUM, 2, 7), (SOBOL_BRIDGE, HIGH, PUT, ONE, 1, 7),
    (SOBOL_QE, USUAL, PUT, MEDIUM, 2, 7), (SOBOL_QE, HIGH, PUT, TWO, 3, 7),
]


def case_id(case):
    draw, model, contract, shape, degree, seed = case
    names = {EULER: "euler", QE: "qe", SOBOL: "sobol", SOBOL_BRIDGE: "sobol-bridge", SOBOL_QE: "sobol-qe"}
    models = {USUAL: "usual", HIGH: "high", EXTREME: "extreme"}
    return f"{names[draw]}-{models[model]}-{'call' if contract[3] else 'put'}-{shape[0]}x{shape[1]}-d{degree}-seed{seed}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_price_is_tied_to_the_oracle_on_the_device_s_matrices(case):
    draw, model, contract, (n_paths, n_steps), degree, seed = case
    st = tie(draw, model, contract, n_paths, n_steps, degree, seed)
    # equal inputs, equal bits -- at 300,001 x 3 whatever U the host picked for the device's compute units
    again = price(draw, model, *contract[:2], contract[2], contract[3], n_paths, n_steps, seed, degree)
    assert (again.sum, again.sumsq, again.n, again.price, again.std_error) == (st.sum, st.sumsq, st.n, st.price, st.std_error)


def test_the_public_method_prices_the_same_bits():
    model, (S, K, q, call), seed = USUAL, PUT, 7
    p = heston_pricer(model)
    for draw, kw in ((EULER, {}), (QE, dict(scheme="qe")), (SOBOL_BRIDGE, dict(method="qmc")),
                     (SOBOL_QE, dict(method="qmc", scheme="qe", path_construction="sequential"))):
        st = price(draw, model, S, K, q, call, 4_097, 13, seed, 2)
        got = p.price_american(S, K, T, R, q, "put", 4_097, 13, 2, seed, True, **kw)
        assert got == (st.price, st.std_error) and st.price > max(K - S, 0.0)
        sp = price(draw, model, S, K, q, call, 4_097, 13, seed, 3, spot_basis=True)
        assert p.price_american(S, K, T, R, q, "put", 4_097, 13, 3, seed, basis="spot", **kw) == sp.price


# ------------------------------------------------------------------------------------------- 2. the spot basis ----
SPOT_CASES = [(EULER, USUAL, PUT, LARGE), (QE, HIGH, CALL, MEDIUM), (SOBOL_BRIDGE, EXTREME, PUT, MEDIUM)]
SPOT_IDS = ["euler", "qe", "sobol-bridge"]


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("draw,model,contract,shape", SPOT_CASES, ids=SPOT_IDS)
def test_the_spot_basis_is_the_one_factor_chain_on_the_heston_spot(draw, model, contract, shape, degree):
    (S, K, q, call), (n_paths, n_steps) = contract, shape
    st = price(draw, model, S, K, q, call, n_paths, n_steps, 7, degree, spot_basis=True)
    spot, _var = matrices(draw, model, S, q, n_paths, n_steps, 7)
    want, x = orc.american_from_paths(spot, K, T, R, "call" if call else "put", degree, return_payoffs=True)
    assert_tied(st, want, x, AMERICAN_TIE)


DEGREE_4_CASES = [(EULER, USUAL, PUT, LARGE, 13), (QE, USUAL, PUT, MEDIUM, 17), (SOBOL_BRIDGE, EXTREME, PUT, MEDIUM, 11)]
REFERENCE_DEGREE_4_GUARD = 0.5 * AMERICAN_TIE_DEGREE_4


@pytest.mark.parametrize("draw,model,contract,shape,seed", DEGREE_4_CASES, ids=SPOT_IDS)
def test_the_spot_basis_of_degree_4(draw, model, contract, shape, seed):
    """AMERICAN_TIE_DEGREE_4's reason, measured for Heston paths on the CPU (NumPy Euler paths, 10,007 .. 20,001 paths x 13 .. 50 dates,
    three seeds each): the reference's lstsq on raw powers of S up to S^4 lies 0 .. 1.4e-3 of the price from a well-conditioned fit of
    the same polynomial space, seed by seed (on the device's matrices: 1.5e-4 .. 1.6e-3 of the price and 1.4e-4 .. 4.1e-3 of the sum
    of squares for the 20,001 x 50 put over six seeds, up to 1.2e-2 of the sum of squares at 10,007 x 13, and 7e-4 .. 5.7e-3 of the price
    for a call at S = 100, K = 95, whose in-the-money spots and their fourth powers are larger: the cases are puts).
    A matrix on which the reference's own error is beyond half the tie says nothing about the device, so the case asserts that first
    (the well-conditioned fit is the oracle's lstsq in the centred, scaled regressor; a seed over the guard was replaced when this file
    was written).  Against that well-conditioned fit the device is tied as at the lower degrees: on those CPU runs the normal equations
    in the library's standardised x and the well-conditioned lstsq give continuation values at most 1.8e-11 apart, far inside GUARD."""
    (S, K, q, call), (n_paths, n_steps) = contract, shape
    typ = "call" if call else "put"
    st = price(draw, model, S, K, q, call, n_paths, n_steps, seed, 4, spot_basis=True)
    spot, var = matrices(draw, model, S, q, n_paths, n_steps, seed)
    want, x = orc.american_from_paths(spot, K, T, R, typ, 4, return_payoffs=True)

    def centred(t, s, v):
        return (s / K - np.mean(s / K)) / np.std(s / K), v

    exact, x_exact, margin = hao.american_from_state(spot, var, K, T, R, model[1], typ, 4, regressors=centred, with_variance=False)
    sumsq, sumsq_exact = float(np.sum(x * x)), float(np.sum(x_exact * x_exact))
    print("device", st.price, st.sumsq, "reference", want, sumsq, "well-conditioned", exact, sumsq_exact, "margin", margin)
    assert abs(want - exact) <= REFERENCE_DEGREE_4_GUARD * exact                       # of what the tie compares: the sum (the price) at rel,
    assert abs(sumsq - sumsq_exact) <= 2 * REFERENCE_DEGREE_4_GUARD * sumsq_exact       # the sum of squares at 2 rel
    assert_tied(st, want, x, AMERICAN_TIE_DEGREE_4)
    assert margin > GUARD
    assert_tied(st, exact, x_exact, AMERICAN_TIE)


# -------------------------------------------------------------------------------------------- 3. the pin rule ----
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_a_constant_variance_pins_every_y_monomial(degree):
    """sigma_v = 0 with v0 = theta: every v_t is theta, every y exactly zero, every monomial with a power of y has a zero pivot and is
    pinned; what is left is the one-factor fit of the same degree on the same spot matrix."""
    model = (2.0, 0.04, 0.0, -0.7, 0.04)
    S, K, q, call = PUT
    spot, var = matrices(EULER, model, S, q, 20_001, 25, 7)
    assert np.all(var == 0.04)
    st = price(EULER, model, S, K, q, call, 20_001, 25, 7, degree)
    want, x = orc.american_from_paths(spot, K, T, R, "put", degree, return_payoffs=True)
    assert_tied(st, want, x, AMERICAN_TIE)


def library_regressors(S, K, q, call, model, n_steps):
    """regressors(t, S_t, v_t) -> (x, y) in the library's own standardisation (olha_regressor_scales: host arithmetic)."""
    kappa, theta, sigma_v, _rho, v0 = model
    cx, wx, cy, wy = _hip.heston_american_scales(S, K, T, R, q, call, kappa, theta, sigma_v, v0, n_steps)
    return lambda t, s, v: ((s / K - cx[t]) / wx[t], (v - cy[t]) / wy[t])


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_a_constant_variance_off_its_mean_pins_every_y_monomial_during_elimination(degree):
    """sigma_v = 0 with v0 = 0.09, not theta: v_t is the same on every path but it is the Euler recursion's value, not the conditional
    mean the regressor is centred on, and the width is at its clamp -- y is a constant in the thousands.  No y column is zero from
    the start: the pivot of y becomes zero only once the constant has been eliminated, x y only after x, and so on, each a cancellation of
    sums of order y^2 .. y^6 down to rounding.  Every monomial with a power of y must pin, and what is left is the one-factor fit.
    First, in NumPy on the same matrices: the restated rule (normal equations in the library's regressors, the pin rule) makes the
    one-factor decisions, none of them within GUARD of its threshold."""
    model = (2.0, 0.04, 0.0, -0.7, 0.09)
    S, K, q, call = PUT
    n_paths, n_steps = 20_001, 25
    spot, var = matrices(EULER, model, S, q, n_paths, n_steps, 7)
    assert np.all(var == var[0]) and np.all(var[0, 1:] != 0.04) and np.all(np.diff(var[0]) < 0)
    regressors = library_regressors(S, K, q, call, model, n_steps)
    y = np.array([regressors(t, spot[:1, t], var[:1, t])[1][0] for t in range(1, n_steps)])
    assert np.all(np.abs(y) > 1.0), y
    report = []
    _price, _cf, _margin, restated = hao.american_from_state(spot, var, K, T, R, model[1], "put", degree, regressors=regressors,
                                                             fit=functools.partial(hao.normal_equations_fit, report=report), return_decisions=True)
    _price, _cf, margin, one_factor = hao.american_from_state(spot, var, K, T, R, model[1], "put", degree, with_variance=False, return_decisions=True)
    unknowns = (degree + 1) * (degree + 2) // 2
    pinned = [sorted(k for k in range(unknowns) if not report[d + k][0] > 1e-11) for d in range(0, len(report), unknowns)]
    print("degree", degree, "margin", margin, "largest pinned ratio", max(r for r, _ in report if not r > 1e-11), "smallest fitted", min(r for r, _ in report if r > 1e-11))
    assert len(pinned) == n_steps - 1 and all(p == [k for k, (a, b) in enumerate((s - b, b) for s in range(degree + 1) for b in range(s + 1)) if b] for p in pinned)
    assert one_factor.any() and np.array_equal(restated, one_factor)
    assert margin > GUARD
    st = price(EULER, model, S, K, q, call, n_paths, n_steps, 7, degree)
    want, x = orc.american_from_paths(spot, K, T, R, "put", degree, return_payoffs=True)
    assert_tied(st, want, x, AMERICAN_TIE)


# -------------------------------------------------------------------- 4. too few paths in the money to regress ----
@pytest.mark.parametrize("draw", [EULER, SOBOL_BRIDGE], ids=["euler", "sobol-bridge"])
def test_five_paths_never_exercise_early(draw):
    S, K, q, call = PUT
    n_steps = 13
    st = price(draw, USUAL, S, K, q, call, 5, n_steps, 7, 2)                 # six unknowns: no date has more than five paths in the money
    spot, var = matrices(draw, USUAL, S, q, 5, n_steps, 7)
    x = np.maximum(K - spot[:, -1], 0.0)
    for _ in range(n_steps):
        x = x * np.exp(-R * (T / n_steps))
    assert np.any(x > 0)
    assert_tied(st, np.mean(x), x, 1e-13)
    assert hao.american_from_state(spot, var, K, T, R, USUAL[1], "put", 2)[2] == math.inf      # the oracle fitted no date either


FEW_N, FEW_SEEDS, FEW_STEPS, FEW_STRIKE = (7, 8, 11, 12, 16, 40), range(12), 6, 110.0
FEW_LEFT_OUT = 0.25


def few_paths_checker(spot, var, degree, regressors):
    """(cash flows, robust) of the restated device algorithm (normal equations, pin rule, the library's regressors) on the matrices.
    ROBUST says that no decision of the run can depend on rounding, by two figures the checker reports about itself:
      pivots   a pivot that follows divisions by pivots of ratio >= rho carries an error of about n^2 u / rho of its diagonal moment (n
               unknowns, u = 2^-53: each entry of the Schur complement has taken at most n updates whose multipliers are known to u / rho, and
               the moments themselves are sums of <= 40 terms in another order); every pivot ratio must lie at least 100 such errors away
               from 1e-11, on either side;
      margin   a backward stable solve errs in the continuation value by about n^2 u K / rho_min (the scaled moment matrix's condition
               number is 1 / rho_min up to a factor n); the smallest |intrinsic - continuation| must be above 100 times that."""
    n, u, report = (degree + 1) * (degree + 2) // 2, 2.0 ** -53, []
    _price, cf, margin = hao.american_from_state(spot, var, FEW_STRIKE, T, R, USUAL[1], "put", degree, regressors=regressors,
                                                 fit=functools.partial(hao.normal_equations_fit, report=report))
    distance = min((abs(ratio - 1e-11) / (n * n * u / floor) for ratio, floor in report), default=math.inf)
    rho_min = min((ratio for ratio, _ in report if ratio > 1e-11), default=1.0)
    return cf, distance >= 100.0 and margin > 100.0 * n * n * u * FEW_STRIKE / rho_min, len(report) // n


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_a_few_paths_where_the_moment_matrix_is_all_but_singular(degree):
    """The two-factor counterpart of test_gpu_exotics' test_american_where_the_moment_matrix_is_singular: 7 .. 40 paths, six dates, a put
    ten in the money, so that dates have exactly NU, NU + 1 or a few more paths in the money (3, 6, 10 unknowns) and the fit all but
    interpolates.  Every price is finite and within [0, K], n ==; wherever the checker's own figures say its decisions are robust the
    device's sum is the checker's at rel 1e-5 (one flipped decision moves it by more).  At most a quarter of the (N, seed) cases may be
    left out that way (counted on the device's matrices when this was written: none of the 72 per degree, 339 / 251 / 120 dates fitted)."""
    S, q, call = 100.0, 0.0, False
    regressors = library_regressors(S, FEW_STRIKE, q, call, USUAL, FEW_STEPS)
    compared = fitted_dates = 0
    for n_paths in FEW_N:
        for seed in FEW_SEEDS:
            st = price(EULER, USUAL, S, FEW_STRIKE, q, call, n_paths, FEW_STEPS, seed, degree)
            spot, var = matrices(EULER, USUAL, S, q, n_paths, FEW_STEPS, seed)
            cf, robust, fitted = few_paths_checker(spot, var, degree, regressors)
            assert st.n == n_paths and math.isfinite(st.price) and 0.0 <= st.price <= FEW_STRIKE, (n_paths, degree, seed, st.price)
            fitted_dates += fitted
            if robust:
                compared += 1
                assert st.sum == pytest.approx(float(np.sum(cf)), rel=1e-5, abs=1e-9), (n_paths, degree, seed, st.sum, float(np.sum(cf)))
    total = len(FEW_N) * len(FEW_SEEDS)
    print("degree", degree, "compared", compared, "of", total, "dates fitted", fitted_dates)
    assert total - compared <= FEW_LEFT_OUT * total
    assert fitted_dates > 0 or degree == 3 and max(FEW_N) <= 10


# ------------------------------------------------------------------------------------------- 5. the statistics ----
@pytest.fixture(scope="module")
def sixteen_seeds():
    """(American, European) prices of the at-the-money put and of the q = 0 call, 16 seeds at 2^14 x 50, degree 2."""
    p = heston_pricer(USUAL)
    out = {}
    for typ in ("put", "call"):
        american = np.array([p.price_american(100.0, 100.0, T, R, 0.0, typ, 1 << 14, 50, 2, seed) for seed in range(100, 116)])
        european = np.array([p.price_monte_carlo(100.0, 100.0, T, R, 0.0, typ, 1 << 14, 50, seed) for seed in range(100, 116)])
        out[typ] = american, european
    return out


def combined_error(a, b):
    return math.sqrt((np.var(a, ddof=1) + np.var(b, ddof=1)) / len(a))


def test_the_american_put_is_not_below_the_european_put(sixteen_seeds):
    american, european = sixteen_seeds["put"]
    print("american", american.mean(), "european", european.mean(), "combined standard error", combined_error(american, european))
    assert american.mean() >= european.mean() - 3 * combined_error(american, european)


def test_the_american_call_without_dividends_is_the_european_call(sixteen_seeds):
    american, european = sixteen_seeds["call"]
    print("american", american.mean(), "european", european.mean(), "combined standard error", combined_error(american, european))
    assert abs(american.mean() - european.mean()) <= 3 * combined_error(american, european)


# --------------------------------------------------------------------------------------------- 6. the refusals ----
def test_every_refusal_leaves_the_context_usable(library):
    _hip.lib()                                                               # a device is up: the refusals still come before any work on it
    for name, args, message in hc.REFUSALS:
        refused(library, getattr(library, name)(*args()), message)
    tie(EULER, USUAL, PUT, 10_007, 13, 2, 7)
    tie(SOBOL_BRIDGE, USUAL, PUT, 10_007, 13, 2, 7)


def test_nan_inputs_give_nan_results():
    for S, K, model in ((float("nan"), 100.0, USUAL), (100.0, float("nan"), USUAL), (100.0, 100.0, (2.0, float("nan"), 0.3, -0.7, 0.04))):
        st = _hip.heston_american_lsm(S, K, T, R, 0.0, False, *model, 1_000, 8, 7, 2)
        assert st.n == 1_000 and math.isnan(st.price) and math.isnan(st.sum) and math.isnan(st.std_error)
