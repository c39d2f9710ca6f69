"""The Heston option surface (include/olmc.h "a Heston option surface", HestonPricer.price_surface, calibrate_heston) on the device.

A cell (strike, step) of one launch is the European payoff at column `step` of HestonPricer.simulate_paths' spot matrix for the same
grid (T, n_steps) and seed or Sobol tables.  The bars are the project's own: TIE for per-path ties of sums, rel 1e-12 for sums that
must add up, four combined standard errors against the reference's fixture (tests/golden/heston_surface.json).

1. Philox: every cell's sums against the NumPy payoffs of the device's own matrix column.
2. The mirror leg: the literal recursion on the negated normals recovered from the device's states.
3. Sobol: against the NumPy oracle of tests/heston_path_oracle.py, both constructions and both legs.
4. Neighbours: olmc_heston / olmc_heston_qmc for the terminal cell, price_monte_carlo on a dyadic grid, price_surface against the matrix.
5. Independence of the cells, shards, determinism, the pinned bits of the existing entry points, profiling, v0 < 0, NaN.
6. The reference at workload level.
7. Calibration: the deterministic conditions only.
"""
import functools
import json
import math
import os

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.black_scholes import implied_volatility
from optionslab_amd.heston import calibrate_heston, calibration_objective
from optionslab_amd.monte_carlo import sobol_tables
from tests import heston_path_oracle as hpo
from tests import gpu_support
from tests.gpu_support import heston_pricer as pricer
from tests.heston_path_oracle import CALM, FELLER_VIOLATING, Q, R, S, T, USUAL

pytestmark = pytest.mark.gpu

TIE = dict(rel=1e-10, abs=1e-12)
STRIKES = (80.0, 100.0, 120.0)
OPTION_TYPES = ("call", "put")


def cells_for(n):
    """(strike, step) cells of an n-step grid, NOT sorted: step 1, step n, a repeated step with two strikes and, from 13 steps on, an
    odd and an even interior step."""
    cells = [(100.0, n), (80.0, 1), (120.0, n), (100.0, 1)]                        # n = 1: four cells of one step
    if n >= 13:
        cells += [(120.0, 8), (100.0, 5), (80.0, 8), (80.0, n - 1), (120.0, n // 2 + 1)]
    return cells


def philox_cells(model, option_type, cells, N, n, seed, antithetic=False, path_offset=0):
    return _hip.heston_surface(S, T, R, Q, option_type == "call", *model, [k for k, _m in cells], [m for _k, m in cells], N, n, seed,
                               antithetic, path_offset)


def sobol_cells(model, option_type, cells, N, n, seed, construction, antithetic=False, point_offset=0):
    sv, shift = sobol_tables(2 * n, seed, point_offset + N)
    return _hip.heston_qmc_surface(S, T, R, Q, option_type == "call", *model, [k for k, _m in cells], [m for _k, m in cells], N, sv, shift,
                                   construction == "bridge", antithetic, point_offset)


def payoff(spot, strike, step, option_type):
    return np.maximum((1.0 if option_type == "call" else -1.0) * (spot[:, step] - strike), 0)


check_sums = functools.partial(gpu_support.check_sums, tie=TIE)


def check_cells(stats, spot_legs, cells, option_type, label):
    """Every cell of one launch against the payoffs of its column, over the given legs' matrices; price and error from those sums."""
    assert len(stats) == len(cells)
    n = spot_legs[0].shape[1] - 1
    for st, (strike, step) in zip(stats, cells):
        x = np.concatenate([payoff(spot, strike, step, option_type) for spot in spot_legs])
        check_sums(st, x, (*label, strike, step, option_type))
        disc = math.exp(-R * step * (T / n))
        assert st.price == pytest.approx(disc * st.sum / st.n, rel=1e-14), label
        # the error through its variance: sumsq / n - mean^2 cancels, so beside rel 1e-6 it carries a few roundings of mean(x^2)
        # (a column whose payoffs are all equal -- step 1 of a start at v0 < 0 -- has variance 0 only up to those)
        variance = (st.std_error / disc) ** 2 * len(x)
        assert variance == pytest.approx(float(np.var(x)), rel=2e-6, abs=16 * 2.0**-52 * float(np.mean(x * x))), label


# ------------------------------------------------------------------------------ 1. Philox: tie to the device's own matrix ----
@pytest.mark.parametrize("n", (1, 2, 13, 64, 252))
def test_philox_cells_match_the_columns_of_the_devices_own_path_matrix(n):
    cells = cells_for(n)
    for mi, model in enumerate((USUAL, FELLER_VIOLATING)):
        p = pricer(model)
        for N in (1, 63, 65, 1000, 4097):
            seed = 100 * n + N + mi
            spot, _var = p.simulate_paths(S, T, R, Q, N, n, seed)
            for option_type in OPTION_TYPES:
                check_cells(philox_cells(model, option_type, cells, N, n, seed), [spot], cells, option_type, (mi, n, N))


# --------------------------------------------------------------------------------------------- 2. Philox: the mirror leg ----
@pytest.mark.parametrize("N,n", [(257, 13), (4096, 64)])
def test_the_antithetic_leg_is_the_recursion_on_the_negated_normals(N, n):
    seed = 17 + n
    spot, var = pricer(CALM).simulate_paths(S, T, R, Q, N, n, seed)
    assert float(var.min()) > 0.0
    z1, z2p = hpo.recovered_normals(spot, var, CALM)
    again, _ = hpo.literal_recursion(z1, z2p, CALM, n)
    assert float(np.max(np.abs(again / spot - 1.0))) < 1e-12                        # the recovery is sound
    mirror, mirror_var = hpo.literal_recursion(-z1, -z2p, CALM, n)
    assert float(mirror_var.min()) > 0.0
    cells = cells_for(n)
    for option_type in OPTION_TYPES:
        plain = philox_cells(CALM, option_type, cells, N, n, seed, antithetic=False)
        both = philox_cells(CALM, option_type, cells, N, n, seed, antithetic=True)
        for a, b, (strike, step) in zip(plain, both, cells):
            x = payoff(mirror, strike, step, option_type)
            print((N, n), strike, step, option_type, "mirror sum", b.sum - a.sum, "oracle", float(np.sum(x)))
            assert a.n == N and b.n == 2 * N
            if float(np.sum(x)) == 0.0:
                assert b.sum == a.sum and b.sumsq == a.sumsq
                continue
            assert b.sum - a.sum == pytest.approx(float(np.sum(x)), rel=1e-10), (strike, step, option_type)
            assert b.sumsq - a.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10), (strike, step, option_type)


# ----------------------------------------------------------------------------------- 3. Sobol: per-path tie to the oracle ----
SOBOL_CASES = [(n, mi, N) for n in (1, 2, 13, 64) for mi in (0, 1) for N in (1, 1000, 1 << 12)]
SOBOL_CASES += [(252, 0, 1000), (1024, 1, 1000)]                                   # once each: a long grid; the bridge's cap


@pytest.mark.parametrize("n,mi,N", SOBOL_CASES, ids=[f"n{c[0]}-model{c[1]}-N{c[2]}" for c in SOBOL_CASES])
def test_sobol_cells_match_the_numpy_oracle(n, mi, N):
    model = (USUAL, FELLER_VIOLATING)[mi]
    seed = 1000 + n + mi
    constructions = ("bridge", "sequential")
    spots = hpo.sobol_spots(n, N, seed, model, constructions)
    cells = cells_for(n)
    for construction in constructions:
        for option_type in OPTION_TYPES:
            for antithetic in (False, True):
                legs = [spots[(construction, leg)] for leg in ((0, 1) if antithetic else (0,))]
                check_cells(sobol_cells(model, option_type, cells, N, n, seed, construction, antithetic), legs, cells, option_type,
                            (n, N, mi, construction, antithetic))


# ------------------------------------------------------------------------------------- 4. agreement with the neighbours ----
def test_the_terminal_cell_alone_has_the_sums_of_the_one_contract_kernels():
    """The drift enters differently (per read-out here, once per path there), so the bits need not match."""
    N, n, seed = 4097, 64, 5
    sv, shift = sobol_tables(2 * n, seed, N)
    for model in (USUAL, FELLER_VIOLATING):
        for strike in STRIKES:
            for is_call in (True, False):
                for antithetic in (False, True):
                    pairs = [(_hip.heston_surface(S, T, R, Q, is_call, *model, [strike], [n], N, n, seed, antithetic)[0],
                              _hip.heston(S, strike, T, R, Q, is_call, *model, N, n, seed, antithetic))]
                    for bridge in (True, False):
                        pairs.append((_hip.heston_qmc_surface(S, T, R, Q, is_call, *model, [strike], [n], N, sv, shift, bridge, antithetic)[0],
                                      _hip.heston_qmc(S, strike, T, R, Q, is_call, *model, N, sv, shift, bridge, antithetic)))
                    for cell, one in pairs:
                        assert cell.n == one.n
                        assert cell.sum == pytest.approx(one.sum, rel=1e-12) and cell.sumsq == pytest.approx(one.sumsq, rel=1e-12)
                        assert cell.price == pytest.approx(one.price, rel=1e-12) and cell.std_error == pytest.approx(one.std_error, rel=1e-9)


def test_on_a_dyadic_grid_a_cell_has_the_sums_of_the_shorter_contract():
    """T = 1, n = 64: dt = T m / 64 / m is exactly 1 / 64 for every m, and the Philox stream of a shorter contract is a prefix."""
    N, n, seed = 4097, 64, 6
    for model in (USUAL, FELLER_VIOLATING):
        for is_call in (True, False):
            cells = [(k, m) for m in (1, 7, 16, 32, 48, 64) for k in (90.0, 110.0)]
            got = _hip.heston_surface(S, T, R, Q, is_call, *model, [k for k, _m in cells], [m for _k, m in cells], N, n, seed)
            for cell, (strike, m) in zip(got, cells):
                one = _hip.heston(S, strike, T * m / 64, R, Q, is_call, *model, N, m, seed)
                assert cell.sum == pytest.approx(one.sum, rel=1e-12) and cell.sumsq == pytest.approx(one.sumsq, rel=1e-12), (strike, m)
                assert cell.price == pytest.approx(one.price, rel=1e-12)


@pytest.mark.parametrize("kw", [dict(), dict(method="qmc"), dict(method="qmc", path_construction="sequential")],
                         ids=["pseudo", "bridge", "sequential"])
def test_price_surface_is_the_discounted_mean_payoff_of_the_matrix_columns(kw):
    N, n, seed = 4097, 64, 21
    maturities = (0.5, 0.25, 1.0, 0.25, 0.015625)                                  # any order, a repeat, one step
    for model in (USUAL, FELLER_VIOLATING):
        p = pricer(model)
        spot, _var = p.simulate_paths(S, T, R, Q, N, n, seed, **kw)
        for option_type in OPTION_TYPES:
            prices = p.price_surface(S, STRIKES, maturities, R, Q, option_type, N, n, seed, **kw)
            again, errors = p.price_surface(S, STRIKES, maturities, R, Q, option_type, N, n, seed, return_error=True, **kw)
            assert prices.shape == errors.shape == (3, 5) and prices.dtype == np.float64 and np.array_equal(prices, again)
            for i, strike in enumerate(STRIKES):
                for j, t_j in enumerate(maturities):
                    x = payoff(spot, strike, round(t_j * n), option_type)
                    disc = math.exp(-R * t_j)
                    assert prices[i, j] == pytest.approx(disc * float(np.mean(x)), rel=1e-10, abs=1e-14), (strike, t_j)
                    assert errors[i, j] == pytest.approx(disc * float(np.std(x)) / math.sqrt(N), rel=1e-6, abs=1e-14), (strike, t_j)
            assert np.array_equal(prices[:, 1], prices[:, 3])


# ------------------------------------------------------------------- 5. independence, shards, determinism, the old bits ----
@pytest.mark.parametrize("kw", [dict(), dict(method="qmc"), dict(method="qmc", path_construction="sequential")],
                         ids=["pseudo", "bridge", "sequential"])
def test_a_cell_does_not_depend_on_its_neighbours_or_its_place(kw):
    """A 5 x 7 surface (35 cells, three launches) against the same cells one per launch, and in reversed order."""
    N, n, seed = 4097, 64, 31
    strikes = (80.0, 90.0, 100.0, 110.0, 120.0)
    maturities = (0.25, 0.5, 1.0, 0.75, 0.5, 0.125, 0.015625)                      # a repeat
    steps = [round(t * n) for t in maturities]
    p = pricer(USUAL)
    prices, errors = p.price_surface(S, strikes, maturities, R, Q, "put", N, n, seed, antithetic=True, return_error=True, **kw)
    if kw:
        sv, shift = sobol_tables(2 * n, seed, N)
        launch = lambda ks, ms: _hip.heston_qmc_surface(S, T, R, Q, False, *USUAL, ks, ms, N, sv, shift, kw.get("path_construction") != "sequential", True)
    else:
        launch = lambda ks, ms: _hip.heston_surface(S, T, R, Q, False, *USUAL, ks, ms, N, n, seed, True)
    cells = [(i, j) for i in range(5) for j in range(7)]
    for i, j in cells:
        st = launch([strikes[i]], [steps[j]])[0]
        assert (st.price, st.std_error) == (prices[i, j], errors[i, j]), (i, j)
    backwards = cells[::-1]
    for a in range(0, 35, 16):
        part = backwards[a:a + 16]
        for (i, j), st in zip(part, launch([strikes[i] for i, _j in part], [steps[j] for _i, j in part])):
            assert (st.price, st.std_error) == (prices[i, j], errors[i, j]), (i, j)


def test_shards_of_one_stream_or_sequence_add_up():
    N, n, a, seed = 4097, 64, 1000, 9                                              # a is no multiple of 64
    cells = cells_for(n)
    for model, option_type, antithetic in ((USUAL, "call", False), (FELLER_VIOLATING, "put", True)):
        calls = [lambda off, cnt: philox_cells(model, option_type, cells, cnt, n, seed, antithetic, off)]
        for construction in ("bridge", "sequential"):
            calls.append(lambda off, cnt, c=construction: sobol_cells(model, option_type, cells, cnt, n, seed, c, antithetic, off))
        for call in calls:
            for whole, lo, hi in zip(call(0, N), call(0, a), call(a, N - a)):
                assert whole.n == lo.n + hi.n == N * (2 if antithetic else 1)
                assert whole.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12)
                assert whole.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12)


def test_equal_seeds_give_equal_bits():
    p = pricer(USUAL)
    maturities = (0.25, 0.5, 1.0)
    for kw in (dict(), dict(method="qmc"), dict(method="qmc", path_construction="sequential")):
        surface = lambda seed, n=64: p.price_surface(S, STRIKES, maturities, R, Q, "call", 4097, n, seed, antithetic=True, **kw)
        first, other = surface(11), surface(12)
        surface(12, 100)                                                            # other tables, another plan, other slabs in between
        assert np.array_equal(surface(11), first) and np.array_equal(surface(12), other) and not np.array_equal(first, other), kw


# Copied from tests/test_gpu_heston_path_payoffs.py: captured before the path-payoff kernels existed.
PINNED = {
    "pseudo_call": "0x1.3e768f52d49d6p+3",
    "pseudo_put_antithetic": "0x1.73332843b5b61p+2",
    "bridge_call": "0x1.370b972c38a65p+3",
    "sequential_put_antithetic": "0x1.74befb3038ddap+2",
    "pseudo_paths": ["0x1.9348bbc2fdfebp+6", "0x1.7ecd18c7a3606p-5", "0x1.a6a38074fba50p+6", "0x1.b06576fc767efp-5"],
    "bridge_paths": ["0x1.7649a92467b64p+6", "0x1.25e0a766a0769p-5", "0x1.16df7b2cac00dp+7", "0x1.a04f6452909c4p-9"],
}


def test_price_monte_carlo_and_simulate_paths_give_the_bits_they_gave_before():
    p = pricer(USUAL)
    K, N, n, seed = 100.0, 4097, 64, 77
    p.price_surface(S, STRIKES, (0.5, 1.0), R, Q, "call", N, n, seed, method="qmc")           # a surface launch first: it leaves nothing behind
    got = {
        "pseudo_call": float(p.price_monte_carlo(S, K, T, R, Q, "call", N, n, seed)).hex(),
        "pseudo_put_antithetic": float(p.price_monte_carlo(S, K, T, R, Q, "put", N, n, seed, True)).hex(),
        "bridge_call": float(p.price_monte_carlo(S, K, T, R, Q, "call", N, n, seed, method="qmc")).hex(),
        "sequential_put_antithetic": float(p.price_monte_carlo(S, K, T, R, Q, "put", N, n, seed, True, method="qmc",
                                                               path_construction="sequential")).hex(),
    }
    for key, kw in (("pseudo_paths", dict()), ("bridge_paths", dict(method="qmc"))):
        spot, var = p.simulate_paths(S, T, R, Q, 1000, n, seed, **kw)
        got[key] = [float(spot[5, 13]).hex(), float(var[5, 13]).hex(), float(spot[999, 64]).hex(), float(var[999, 64]).hex()]
    print(json.dumps(got))
    assert got == PINNED


def test_with_profiling_on_the_launch_counts_once_in_the_kernel_time():
    N, n = 1000, 64
    cells = cells_for(n)
    calls = [lambda: philox_cells(USUAL, "call", cells, N, n, 1, True)]
    for construction in ("bridge", "sequential"):
        calls.append(lambda c=construction: sobol_cells(USUAL, "put", cells, N, n, 1, c, True))
    _hip.profile_enable(True)
    try:
        for call in calls:
            _hip.profile_reset()
            call()
            launches, ms = _hip.kernel_time()
            assert launches == 1 and ms > 0.0
    finally:
        _hip.profile_enable(False)
    _hip.profile_reset()


def test_a_negative_start_variance_and_nan_inputs_at_the_c_abi():
    """v0 < 0 means what it means in olmc_heston (the first step is deterministic).  A NaN in S, T, r, q or the model answers NaN in every
    cell, a NaN strike in its own cell only."""
    model, N, n, seed = (2.0, 0.04, 0.3, -0.7, -0.01), 1000, 13, 3
    cells = cells_for(n)
    spot, var = _hip.heston_paths(S, T, R, Q, *model, N, n, seed, path_major=True)
    assert np.all(var[:, 0] == -0.01) and np.all(spot[:, 1] == spot[0, 1])
    sv, shift = sobol_tables(2 * n, seed, N)
    for option_type in OPTION_TYPES:
        check_cells(philox_cells(model, option_type, cells, N, n, seed), [spot], cells, option_type, ("v0 < 0",))
        for construction in ("bridge", "sequential"):
            qspot, _ = _hip.heston_qmc_paths(S, T, R, Q, *model, N, sv, shift, construction == "bridge", path_major=True)
            check_cells(sobol_cells(model, option_type, cells, N, n, seed, construction), [qspot], cells, option_type, ("v0 < 0", construction))
    nan = float("nan")
    strikes, steps = [80.0, nan, 120.0], [13, 5, 5]
    clean = _hip.heston_surface(S, T, R, Q, True, *USUAL, [80.0, 100.0, 120.0], steps, N, n, seed)
    for got in (_hip.heston_surface(S, T, R, Q, True, *USUAL, strikes, steps, N, n, seed),
                _hip.heston_qmc_surface(S, T, R, Q, True, *USUAL, strikes, steps, N, sv, shift)):
        assert math.isnan(got[1].price) and math.isnan(got[1].std_error) and math.isfinite(got[0].price) and math.isfinite(got[2].price)
    got = _hip.heston_surface(S, T, R, Q, True, *USUAL, strikes, steps, N, n, seed)
    assert (got[0].price, got[2].price) == (clean[0].price, clean[2].price)
    for args in ((nan, T, R, Q, True, *USUAL), (S, nan, R, Q, True, *USUAL), (S, T, nan, Q, True, *USUAL), (S, T, R, nan, True, *USUAL),
                 (S, T, R, Q, True, nan, *USUAL[1:]), (S, T, R, Q, True, *USUAL[:4], nan)):
        assert all(math.isnan(st.price) for st in _hip.heston_surface(*args, [80.0, 100.0, 120.0], steps, N, n, seed))
        assert all(math.isnan(st.price) for st in _hip.heston_qmc_surface(*args, [80.0, 100.0, 120.0], steps, N, sv, shift))


# ------------------------------------------------------------------------------------- 6. the reference at workload level ----
def test_prices_agree_with_the_reference_at_workload_level():
    """The reference's price_monte_carlo cell by cell (N = 100 000, a NumPy seed; tests/golden/make_heston_surface.py): each of the 36
    prices within 4 combined standard errors, once on Philox paths and once on Sobol points.  72 comparisons at four standard errors
    raise a false alarm about 0.5 % of the time for a fresh seed; the seeds are fixed, so the outcome is deterministic thereafter."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heston_surface.json")) as f:
        doc = json.load(f)
    models = {k: tuple(v) for k, v in doc["models"].items()}
    inp = doc["inputs"]
    n, strikes = inp["n_steps"], inp["strikes"]
    maturities = [inp["T"] * m / n for m in inp["steps"]]
    for kw in (dict(n_paths=200_000, seed=2024), dict(n_paths=1 << 14, seed=2024, method="qmc")):
        for model_name, model in models.items():
            for option_type in OPTION_TYPES:
                prices, errors = pricer(model).price_surface(inp["S"], strikes, maturities, inp["r"], inp["q"], option_type, n_steps=n,
                                                             return_error=True, **kw)
                rows = [row for row in doc["prices"] if row["model"] == model_name and row["option_type"] == option_type]
                assert len(rows) == 9
                for row in rows:
                    i, j = strikes.index(row["strike"]), inp["steps"].index(row["step"])
                    bound = 4.0 * math.hypot(errors[i, j], row["std_error"])
                    print(kw.get("method", "pseudo"), model_name, option_type, row["strike"], row["step"], prices[i, j], row["price"],
                          "distance / bound", abs(prices[i, j] - row["price"]) / bound)
                    assert abs(prices[i, j] - row["price"]) <= bound, (kw, row, prices[i, j], errors[i, j])


# ------------------------------------------------------------------------------------------------------ 7. calibration ----
def test_calibration_is_deterministic_and_prices_one_surface_per_evaluation():
    """Quotes made by the model itself at USUAL: with the same seed and settings the objective there is exactly 0; from the reference's
    default start (rho = -0.5) the optimiser does not end above where it began; every objective evaluation is one surface launch.  How
    closely L-BFGS-B recovers USUAL is not asserted (DESIGN.md has the measured run)."""
    strikes, maturities = (90.0, 100.0, 110.0), (0.25, 0.5, 1.0)
    settings = dict(n_paths=1 << 14, n_steps=64, seed=7)
    prices = pricer(USUAL).price_surface(S, strikes, maturities, R, Q, "call", method="qmc", **settings)
    ivs = [[implied_volatility(float(prices[i, j]), S, strikes[i], maturities[j], R, "call", Q) for j in range(3)] for i in range(3)]
    market = dict(spot=S, strikes=strikes, maturities=maturities, market_ivs=ivs, r=R, q=Q)
    objective = calibration_objective(market, **settings)
    assert objective(USUAL) == 0.0 and objective.evals == 1
    start = objective((2.0, 0.04, 0.3, -0.5, 0.04))
    assert 0.0 < start < 1.0
    assert objective(USUAL) == 0.0                                                   # after another model's surface
    _hip.profile_enable(True)
    try:
        _hip.profile_reset()
        fitted = calibrate_heston(market, maxiter=3, **settings)
        launches, _ms = _hip.kernel_time()
    finally:
        _hip.profile_enable(False)
    _hip.profile_reset()
    print("after 3 iterations:", fitted, "error", fitted.calibration_error, "surfaces", fitted.calibration_evals, "launches", launches)
    assert isinstance(fitted, ol.HestonPricer)
    assert math.isfinite(fitted.calibration_error) and fitted.calibration_error <= start
    assert fitted.calibration_evals >= 6 and launches == fitted.calibration_evals             # nine cells: one launch per surface
