"""Heston scenario sets and the fused finite-difference Greeks (include/olmc.h "Heston scenario sets and finite-difference Greeks",
HestonPricer.price_scenarios, HestonMCAdapter) on the device.

Scenario i of a launch is the European contract olmc_heston / olmc_heston_qmc price with its parameters, the same n_steps and the same
seed or Sobol tables.  The bars are the project's own (tests/test_gpu_heston_surface.py): TIE for per-path ties of sums against NumPy,
rel 1e-12 for sums that must agree with a neighbouring kernel or add up, == where bits must not change, five combined standard errors
against the reference's fixture (tests/golden/heston_greeks.json).

 1. Philox: every scenario's sums against the NumPy payoffs of the device's own path matrix for its parameters.
 2. The mirror leg: the literal recursion on the negated normals recovered from the device's states.
 3. Sobol: against the NumPy oracle of tests/heston_scenario_oracle.py, both constructions and both legs.
 4. Neighbours: each scenario alone against olmc_heston / olmc_heston_qmc.
 5. Independence of the scenarios, of their order and of the cut into launches.
 6. Shards.  7. Determinism and the pinned bits of the existing entry points.
 8. Fused = literal Greeks.  9. One launch.  10. NaN.  11. The reference at workload level.
"""
import copy
import json
import math
import os

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.greeks import compute_greeks_unified, fd_steps
from optionslab_amd.monte_carlo import sobol_tables
from tests import heston_scenario_oracle as hso
from tests.gpu_support import heston_pricer as pricer
from tests.heston_path_oracle import CALM, FELLER_VIOLATING, USUAL

pytestmark = pytest.mark.gpu

TIE = dict(rel=1e-10, abs=1e-12)
S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.02
MODELS = (USUAL, FELLER_VIOLATING)
KINDS = ("pseudo", "bridge", "sequential")
GREEK_NAMES = ("price", "delta", "gamma", "vega", "theta", "rho", "vanna", "charm", "vomma")


def scenario(S_=S, K_=K, T_=T, r_=R, q_=Q, call=True, model=USUAL):
    """_hip's tuple: (S, K, T, r, q, is_call, kappa, theta, sigma_v, rho, v0)."""
    return (S_, K_, T_, r_, q_, call, *model)


def as_mapping(sc):
    S_, K_, T_, r_, q_, call, kappa, theta, sigma_v, rho, v0 = sc
    return dict(S=S_, K=K_, T=T_, r=r_, q=q_, option_type="call" if call else "put", kappa=kappa, theta=theta, sigma_v=sigma_v, rho=rho, v0=v0)


def greeks_bumps(sigma, T_=T, second=True):
    """(S, T, r, sigma) of compute_greeks_unified's evaluations in its call order."""
    h_S, h_v, h_r, h_T = fd_steps(S)
    has_T = T_ > h_T
    bumps = [(S, T_, R, sigma), (S + h_S, T_, R, sigma), (S - h_S, T_, R, sigma), (S, T_, R, sigma + h_v), (S, T_, R, sigma - h_v)]
    if has_T:
        bumps.append((S, T_ - h_T, R, sigma))
    bumps += [(S, T_, R + h_r, sigma), (S, T_, R - h_r, sigma)]
    if second:
        bumps += [(S + h_S, T_, R, sigma + h_v), (S + h_S, T_, R, sigma - h_v), (S - h_S, T_, R, sigma + h_v), (S - h_S, T_, R, sigma - h_v)]
        if has_T:
            bumps += [(S + h_S, T_ - h_T, R, sigma), (S - h_S, T_ - h_T, R, sigma)]
    return bumps


def greeks_set(model):
    """GREEKS: the 14 contracts for a call at sigma = sqrt(v0), sigma -> v0 = sigma^2."""
    return [scenario(S_=s, T_=t, r_=r, model=(*model[:4], v * v)) for s, t, r, v in greeks_bumps(math.sqrt(model[4]))]


def mixed_set(model):
    """MIXED: 16 scenarios of 6 recursions, unsorted, calls and puts; spots, strikes, rates and q differ within a recursion (6 and 7 share
    their spot and rates and differ in strike and call / put: one exponential serves both); A and B differ in T only; D starts at v0 < 0."""
    kappa, theta, sigma_v, rho, v0 = model
    recursions = {"A": (1.0, model), "B": (0.5, model), "C": (1.0, (kappa + 1.0, theta, sigma_v, rho, v0)),
                  "D": (1.0, (kappa, theta, sigma_v, rho, -0.01)), "E": (0.75, (kappa, theta, 1.2 * sigma_v, -rho, v0)),
                  "F": (2.0, (kappa, 1.5 * theta, sigma_v, rho, 1.5 * v0))}
    out = []
    for i, name in enumerate("CADBFEAADCBBEFCA"):
        T_, m = recursions[name]
        out.append(scenario(95.0 + i, 90.0 + 2.5 * (i % 9), T_, 0.01 * (i % 4), 0.005 * (i % 3), i % 3 != 0, m))
    out[7] = scenario(out[6][0], 104.0, out[6][2], out[6][3], out[6][4], not out[6][5], out[6][6:])
    return out


def test_the_sets_are_what_the_tests_below_take_them_for():
    for model in MODELS:
        assert _hip.heston_scenario_layout(greeks_set(model)) == (4, [0, 0, 0, 1, 2, 3, 0, 0, 1, 2, 1, 2, 3, 3])
        n_rec, group = _hip.heston_scenario_layout(mixed_set(model))
        assert n_rec == 6 and group == ["CADBFE".index(c) for c in "CADBFEAADCBBEFCA"]


def launch(kind, scenarios, N, n, seed, antithetic=False, offset=0, tables=None):
    if kind == "pseudo":
        return _hip.heston_scenarios(scenarios, N, n, seed, antithetic, offset)
    sv, shift = tables if tables is not None else sobol_tables(2 * n, seed, offset + N)
    return _hip.heston_qmc_scenarios(scenarios, N, sv, shift, kind == "bridge", antithetic, offset)


def check_stats(st, x, sc, label):
    """A scenario's sums against the payoffs x of its paths; price and error from those sums."""
    want, want2 = float(np.sum(x)), float(np.sum(x * x))
    print(label, "sum", st.sum, "oracle", want, "sumsq", st.sumsq, "oracle", want2)
    assert st.n == len(x), label
    assert st.sum == pytest.approx(want, **TIE), label
    assert st.sumsq == pytest.approx(want2, **TIE), label
    disc = math.exp(-sc[3] * sc[2])
    assert st.price == pytest.approx(disc * st.sum / st.n, rel=1e-14), label
    # the error through its variance: sumsq / n - mean^2 cancels, so beside rel 2e-6 it carries a few roundings of mean(x^2)
    variance = (st.std_error / disc) ** 2 * len(x)
    assert variance == pytest.approx(float(np.var(x)), rel=2e-6, abs=16 * 2.0**-52 * float(np.mean(x * x))), label


def device_paths(sc, N, n, seed, cache):
    key = (sc[0], *sc[2:5], *sc[6:])
    if key not in cache:
        cache[key] = _hip.heston_paths(sc[0], sc[2], sc[3], sc[4], *sc[6:], N, n, seed, path_major=True)
    return cache[key]


# ------------------------------------------------------------------------------ 1. Philox: tie to the device's own matrix ----
@pytest.mark.parametrize("n", (1, 2, 13, 64))
def test_philox_scenarios_match_the_last_column_of_the_devices_own_path_matrices(n):
    for mi, model in enumerate(MODELS):
        for N in (1, 63, 65, 1000, 4097):
            seed = 100 * n + N + mi
            cache = {}
            for name, scenarios in (("greeks", greeks_set(model)), ("mixed", mixed_set(model))):
                stats = launch("pseudo", scenarios, N, n, seed)
                assert len(stats) == len(scenarios)
                for i, (st, sc) in enumerate(zip(stats, scenarios)):
                    spot, _var = device_paths(sc, N, n, seed, cache)
                    check_stats(st, hso.payoff(spot[:, n], sc), sc, (name, mi, n, N, i))


# --------------------------------------------------------------------------------------------- 2. Philox: the mirror leg ----
CALM_OTHER = (1.5, 0.09, 0.1, -0.5, 0.1)
CALM_SET = [scenario(model=CALM), scenario(105.0, 95.0, 1.0, 0.03, 0.0, False, CALM), scenario(100.0, 110.0, 0.5, R, Q, True, CALM),
            scenario(98.0, 100.0, 0.5, R, 0.0, False, CALM), scenario(model=CALM_OTHER), scenario(100.0, 90.0, 1.0, 0.0, 0.01, False, CALM_OTHER)]


@pytest.mark.parametrize("N,n", [(257, 13), (4096, 64)])
def test_the_antithetic_leg_is_the_recursion_on_the_negated_normals(N, n):
    seed = 17 + n
    plain = launch("pseudo", CALM_SET, N, n, seed, antithetic=False)
    both = launch("pseudo", CALM_SET, N, n, seed, antithetic=True)
    cache = {}
    for a, b, sc in zip(plain, both, CALM_SET):
        S_, _K, T_, r_, q_, _c, *model = sc
        spot, var = device_paths(sc, N, n, seed, cache)
        assert float(var.min()) > 0.0
        z1, z2p = hso.recovered_normals(spot, var, model, T_, r_, q_)
        again, _ = hso.literal_recursion(z1, z2p, model, n, S_, T_, r_, q_)
        assert float(np.max(np.abs(again / spot - 1.0))) < 1e-12                    # the recovery is sound
        mirror, mirror_var = hso.literal_recursion(-z1, -z2p, model, n, S_, T_, r_, q_)
        assert float(mirror_var.min()) > 0.0
        x = hso.payoff(mirror[:, n], sc)
        print((N, n), sc, "mirror sum", b.sum - a.sum, "oracle", float(np.sum(x)))
        assert a.n == N and b.n == 2 * N and float(np.sum(x)) > 0.0
        assert b.sum - a.sum == pytest.approx(float(np.sum(x)), rel=1e-10), sc
        assert b.sumsq - a.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10), sc


# ----------------------------------------------------------------------------------- 3. Sobol: per-path tie to the oracle ----
SOBOL_CASES = [(n, mi, N) for n in (1, 2, 13, 64) for mi in (0, 1) for N in (1, 1000, 1 << 12)]
SOBOL_CASES += [(252, 0, 1000), (1024, 1, 1000)]                                   # once each: a long grid; the bridge's cap


@pytest.mark.parametrize("n,mi,N", SOBOL_CASES, ids=[f"n{c[0]}-model{c[1]}-N{c[2]}" for c in SOBOL_CASES])
def test_sobol_scenarios_match_the_numpy_oracle(n, mi, N):
    model = MODELS[mi]
    seed = 1000 + n + mi
    constructions = ("bridge", "sequential")
    normals = hso.sobol_step_normals(n, N, seed, constructions)
    tables = sobol_tables(2 * n, seed, N)
    sets = [("mixed", mixed_set(model))] + ([("greeks", greeks_set(model))] if n <= 64 else [])
    for construction in constructions:
        spots = {}
        for name, scenarios in sets:
            for antithetic in (False, True):
                stats = launch(construction, scenarios, N, n, seed, antithetic, tables=tables)
                for i, (st, sc) in enumerate(zip(stats, scenarios)):
                    key = (sc[0], *sc[2:5], *sc[6:])
                    if key not in spots:
                        spots[key] = hso.terminal_spots(normals[construction], sc, n, legs=(0, 1))
                    x = hso.payoff(spots[key] if antithetic else spots[key][:N], sc)
                    check_stats(st, x, sc, (name, n, N, mi, construction, antithetic, i))


# ------------------------------------------------------------------------------------- 4. agreement with the neighbours ----
def test_each_scenario_alone_has_the_sums_of_the_one_contract_kernels():
    """The drift enters differently (after the loop here, inside the sum there), so the bits need not match."""
    N, n, seed = 4097, 64, 5
    sv, shift = sobol_tables(2 * n, seed, N)
    for model in MODELS:
        for sc in greeks_set(model) + mixed_set(model):
            for antithetic in (False, True):
                pairs = [(_hip.heston_scenarios([sc], N, n, seed, antithetic)[0], _hip.heston(*sc, N, n, seed, antithetic))]
                for bridge in (True, False):
                    pairs.append((_hip.heston_qmc_scenarios([sc], N, sv, shift, bridge, antithetic)[0],
                                  _hip.heston_qmc(*sc, N, sv, shift, bridge, antithetic)))
                for got, one in pairs:
                    assert got.n == one.n
                    assert got.sum == pytest.approx(one.sum, rel=1e-12) and got.sumsq == pytest.approx(one.sumsq, rel=1e-12), sc
                    assert got.price == pytest.approx(one.price, rel=1e-12) and got.std_error == pytest.approx(one.std_error, rel=1e-9), sc


@pytest.mark.parametrize("kw", [dict(), dict(method="qmc"), dict(method="qmc", path_construction="sequential")], ids=KINDS)
def test_price_scenarios_is_price_monte_carlo_scenario_by_scenario(kw):
    N, n, seed = 4097, 64, 21
    p = pricer(USUAL)
    scenarios = [dict(S=S, K=K, T=T, r=R), dict(S=S, K=90.0, T=0.5, r=R, q=Q, option_type="put"), dict(S=S, K=K, T=T, r=R, q=Q, v0=0.09),
                 dict(S=101.0, K=K, T=T, r=0.0, kappa=1.0, theta=0.05, sigma_v=0.5, rho=0.2)]
    prices, errors = p.price_scenarios(scenarios, N, n, seed, True, return_error=True, **kw)
    assert prices.shape == errors.shape == (4,) and prices.dtype == np.float64
    assert np.array_equal(prices, p.price_scenarios(scenarios, N, n, seed, True, **kw))
    for i, sc in enumerate(scenarios):
        one = copy.copy(p)
        for key in ("kappa", "theta", "sigma_v", "rho", "v0"):
            setattr(one, key, sc.get(key, getattr(p, key)))
        want, want_error = one.price_monte_carlo(sc["S"], sc["K"], sc["T"], sc["r"], sc.get("q", 0.0), sc.get("option_type", "call"), N, n, seed, True,
                                                 return_error=True, **kw)
        assert prices[i] == pytest.approx(float(want), rel=1e-12) and errors[i] == pytest.approx(want_error, rel=1e-9), sc
    assert (p.kappa, p.theta, p.sigma_v, p.rho, p.v0) == USUAL


# ------------------------------------------------------------------------------------------------------ 5. independence ----
@pytest.mark.parametrize("kind", KINDS)
def test_a_scenario_does_not_depend_on_its_neighbours_its_place_or_the_cut(kind):
    N, n, seed = 4097, 64, 31
    tables = sobol_tables(2 * n, seed, N)
    for model in MODELS:
        scenarios = mixed_set(model)
        whole = launch(kind, scenarios, N, n, seed, True, tables=tables)
        bits = [(st.sum, st.sumsq, st.n, st.price, st.std_error) for st in whole]
        for i, sc in enumerate(scenarios):                                          # alone: one recursion, in slot 0
            st = launch(kind, [sc], N, n, seed, True, tables=tables)[0]
            assert (st.sum, st.sumsq, st.n, st.price, st.std_error) == bits[i], (kind, i)
        for st, want in zip(launch(kind, scenarios[::-1], N, n, seed, True, tables=tables), bits[::-1]):      # other slots, other recursion numbers
            assert (st.sum, st.sumsq, st.n, st.price, st.std_error) == want, kind
        pair = launch(kind, [scenarios[4], scenarios[1]], N, n, seed, True, tables=tables)                     # two of the six recursions
        assert [(st.sum, st.sumsq) for st in pair] == [bits[4][:2], bits[1][:2]]
        # a seventh recursion appended: price_scenarios cuts the list into two launches
        seventh = scenario(S, K, 1.25, R, Q, True, model)
        kw = dict() if kind == "pseudo" else dict(method="qmc", path_construction=kind)
        prices, errors = pricer(USUAL).price_scenarios([as_mapping(sc) for sc in scenarios + [seventh]], N, n, seed, True, return_error=True, **kw)
        assert [(p, e) for p, e in zip(prices[:16], errors[:16])] == [(b[3], b[4]) for b in bits], kind
        alone = launch(kind, [seventh], N, n, seed, True, tables=tables)[0]
        assert (prices[16], errors[16]) == (alone.price, alone.std_error)


# ------------------------------------------------------------------------------------------------------------ 6. shards ----
def test_shards_of_one_stream_or_sequence_add_up():
    N, n, a, seed = 4097, 64, 1000, 9                                              # a is no multiple of 64
    for model, antithetic in ((USUAL, False), (FELLER_VIOLATING, True)):
        scenarios = mixed_set(model)
        for kind in KINDS:
            call = lambda off, cnt: launch(kind, scenarios, cnt, n, seed, antithetic, off)
            for whole, lo, hi, sc in zip(call(0, N), call(0, a), call(a, N - a), scenarios):
                assert whole.n == lo.n + hi.n == N * (2 if antithetic else 1)
                assert whole.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12), (kind, sc)
                assert whole.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12), (kind, sc)
                combined = _hip.combine_stats([(lo.sum, lo.sumsq, lo.n), (hi.sum, hi.sumsq, hi.n)], sc[3], sc[2])     # the scenario's own r, T
                assert combined.price == pytest.approx(whole.price, rel=1e-12)


# ------------------------------------------------------------------------------------- 7. determinism and the old bits ----
def test_equal_seeds_give_equal_bits():
    scenarios = mixed_set(USUAL)
    for kind in KINDS:
        run = lambda seed, n=64, N=4097: [(st.sum, st.sumsq) for st in launch(kind, scenarios, N, n, seed, True)]
        first, other = run(11), run(12)
        run(12, 100, 1000)                                                          # another grid, other tables, another plan, other slabs in between
        assert run(11) == first and run(12) == other and first != other, kind


# Copied from tests/test_gpu_heston_surface.py (there from tests/test_gpu_heston_path_payoffs.py): captured before those kernels existed.
PINNED = {
    "pseudo_call": "0x1.3e768f52d49d6p+3",
    "pseudo_put_antithetic": "0x1.73332843b5b61p+2",
    "bridge_call": "0x1.370b972c38a65p+3",
    "sequential_put_antithetic": "0x1.74befb3038ddap+2",
    "pseudo_paths": ["0x1.9348bbc2fdfebp+6", "0x1.7ecd18c7a3606p-5", "0x1.a6a38074fba50p+6", "0x1.b06576fc767efp-5"],
    "bridge_paths": ["0x1.7649a92467b64p+6", "0x1.25e0a766a0769p-5", "0x1.16df7b2cac00dp+7", "0x1.a04f6452909c4p-9"],
}


def test_price_monte_carlo_and_simulate_paths_give_the_bits_they_gave_before():
    from tests.heston_path_oracle import Q as Q0, R as R0                           # the pinned bits' own rates
    p = pricer(USUAL)
    K0, N, n, seed = 100.0, 4097, 64, 77
    for kind in KINDS:                                                              # scenario launches first: they leave nothing behind
        launch(kind, mixed_set(USUAL), N, n, seed, True)
    got = {
        "pseudo_call": float(p.price_monte_carlo(S, K0, T, R0, Q0, "call", N, n, seed)).hex(),
        "pseudo_put_antithetic": float(p.price_monte_carlo(S, K0, T, R0, Q0, "put", N, n, seed, True)).hex(),
        "bridge_call": float(p.price_monte_carlo(S, K0, T, R0, Q0, "call", N, n, seed, method="qmc")).hex(),
        "sequential_put_antithetic": float(p.price_monte_carlo(S, K0, T, R0, Q0, "put", N, n, seed, True, method="qmc",
                                                               path_construction="sequential")).hex(),
    }
    for key, kw in (("pseudo_paths", dict()), ("bridge_paths", dict(method="qmc"))):
        spot, var = p.simulate_paths(S, T, R0, Q0, 1000, n, seed, **kw)
        got[key] = [float(spot[5, 13]).hex(), float(var[5, 13]).hex(), float(spot[999, 64]).hex(), float(var[999, 64]).hex()]
    print(json.dumps(got))
    assert got == PINNED


# ------------------------------------------------------------------------------------------------- 8. fused = literal ----
def finite_differences(P, T_, second):
    """compute_greeks_unified's formulas over the prices P of greeks_bumps' evaluations, in that order."""
    h_S, h_v, h_r, h_T = fd_steps(S)
    has_T = T_ > h_T
    it = iter(P)
    mid, s_up, s_dn, v_up, v_dn = (next(it) for _ in range(5))
    t_dn = next(it) if has_T else None
    r_up, r_dn = next(it), next(it)
    delta = (s_up - s_dn) / (2 * h_S)
    out = [mid, delta, (s_up - 2 * mid + s_dn) / (h_S * h_S), (v_up - v_dn) / (2 * h_v),
           (t_dn - mid) / h_T if has_T else -mid / max(T_, 1e-6), (r_up - r_dn) / (2 * h_r)]
    if second:
        uu, ud, du, dd = (next(it) for _ in range(4))
        out.append((uu - ud - du + dd) / (4 * h_S * h_v))
        out.append(((next(it) - next(it)) / (2 * h_S) - delta) / h_T if has_T else 0.0)
        out.append((v_up - 2 * mid + v_dn) / (h_v * h_v))
    return out


class Recording(ol.HestonMCAdapter):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def price(self, S_, K_, T_, r_, sigma, option_type, q=0.0, **kw):
        value = super().price(S_, K_, T_, r_, sigma, option_type, q, **kw)
        self.calls.append(((S_, T_, r_, sigma), float(value)))
        return value


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T_,second", [(1.0, True), (1.0, False), (1 / 400, True)], ids=["second-order", "first-order", "short"])
def test_the_fused_greeks_are_the_literal_ones(kind, T_, second):
    N, n, seed, sigma = 4097, 64, 41, 0.25
    kw = dict() if kind == "pseudo" else dict(method="qmc", path_construction=kind)
    for model, option_type, antithetic in ((USUAL, "call", False), (FELLER_VIOLATING, "put", True)):
        p = pricer(model)
        is_call = option_type == "call"
        if kind == "pseudo":
            out9, evals = _hip.heston_greeks_fd(S, K, T_, R, sigma, Q, is_call, *model[:4], N, n, seed, antithetic, second, want_evals=True)
        else:
            sv, shift = sobol_tables(2 * n, seed, N)
            out9, evals = _hip.heston_qmc_greeks_fd(S, K, T_, R, sigma, Q, is_call, *model[:4], N, sv, shift, kind == "bridge", antithetic, second,
                                                    want_evals=True)
        bumps = greeks_bumps(sigma, T_, second)
        assert len(evals) == 14 and len(bumps) == {(1.0, True): 14, (1.0, False): 8, (1 / 400, True): 11}[(T_, second)]
        for st in evals[len(bumps):]:
            assert (st.sum, st.sumsq, st.n, st.price, st.std_error) == (0.0, 0.0, 0, 0.0, 0.0)
        # the 14 literal price_monte_carlo calls with the same seed or tables
        for st, (s, t, r, v) in zip(evals, bumps):
            one = copy.copy(p)
            one.v0 = v**2
            want, want_error = one.price_monte_carlo(s, K, t, r, Q, option_type, N, n, seed, antithetic, return_error=True, **kw)
            assert st.n == N * (2 if antithetic else 1)
            assert st.price == pytest.approx(float(want), rel=1e-12) and st.std_error == pytest.approx(want_error, rel=1e-9), (s, t, r, v)
        want9 = finite_differences([st.price for st in evals], T_, second)
        assert list(out9[:len(want9)]) == want9
        # the adapter: one launch, the same nine numbers; fused=False the 14-call way
        adapter = Recording(p, N, n, seed, antithetic, **kw)
        fused = compute_greeks_unified(adapter, S, K, T_, R, sigma, option_type, Q, second)
        assert list(fused) == list(GREEK_NAMES[:len(want9)]) and [float(v) for v in fused.values()] == want9 and adapter.calls == []
        literal = compute_greeks_unified(adapter, S, K, T_, R, sigma, option_type, Q, second, fused=False)
        assert [c[0] for c in adapter.calls] == bumps
        for (_bump, value), st in zip(adapter.calls, evals):
            assert value == pytest.approx(st.price, rel=1e-12)
        for name, value, want in zip(fused, literal.values(), want9):
            assert float(value) == pytest.approx(want, rel=1e-6, abs=1e-6 * abs(want9[0])), name      # differences of prices that agree to 1e-12
        if T_ < 1 / 365:
            assert fused["theta"] == -fused["price"] / T_ and fused["charm"] == 0.0
        assert p.v0 == model[4]                                                     # the wrapped pricer is untouched
        if kind == "pseudo" and T_ == 1.0 and second:
            wrapped = ol.greeks_heston_monte_carlo(p, S, K, T_, R, sigma, option_type, Q, n_paths=N, n_steps=n, seed=seed, antithetic=antithetic)
            assert [float(v) for v in wrapped.values()] == want9
            at_v0 = ol.greeks_heston_monte_carlo(p, S, K, T_, R, None, option_type, Q, n_paths=N, n_steps=n, seed=seed)
            assert at_v0["price"] == pytest.approx(float(p.price_monte_carlo(S, K, T_, R, Q, option_type, N, n, seed)), rel=1e-12)


# ------------------------------------------------------------------------------------------------------ 9. one launch ----
def test_with_profiling_on_every_entry_point_counts_once_in_the_kernel_time():
    N, n, seed = 1000, 64, 1
    sv, shift = sobol_tables(2 * n, seed, N)
    scenarios = mixed_set(USUAL)
    calls = [lambda: _hip.heston_scenarios(scenarios, N, n, seed, True),
             lambda: _hip.heston_greeks_fd(S, K, T, R, 0.2, Q, True, *USUAL[:4], N, n, seed, True, True)]
    for bridge in (True, False):
        calls.append(lambda b=bridge: _hip.heston_qmc_scenarios(scenarios, N, sv, shift, b, True))
        calls.append(lambda b=bridge: _hip.heston_qmc_greeks_fd(S, K, T, R, 0.2, Q, False, *USUAL[:4], N, sv, shift, b, True, True, want_evals=False))
    _hip.profile_enable(True)
    try:
        for call in calls:
            _hip.profile_reset()
            call()
            launches, ms = _hip.kernel_time()
            assert launches == 1 and ms > 0.0
        _hip.profile_reset()
        _hip.heston_scenario_layout(scenarios)                                       # host arithmetic: no launch
        assert _hip.kernel_time()[0] == 0
    finally:
        _hip.profile_enable(False)
    _hip.profile_reset()


# ------------------------------------------------------------------------------------------------------------- 10. NaN ----
def test_a_nan_poisons_its_own_scenario_only():
    N, n, seed = 1000, 13, 3
    nan = float("nan")
    base = [scenario(), scenario(101.0, 95.0, 0.5, 0.03, 0.01, False, USUAL), scenario(model=FELLER_VIOLATING),
            scenario(99.0, 105.0, 1.0, R, Q, False, (2.0, 0.04, 0.3, -0.7, -0.01)), scenario(K_=110.0)]
    sv, shift = sobol_tables(2 * n, seed, N)
    for run in (lambda s: _hip.heston_scenarios(s, N, n, seed, True), lambda s: _hip.heston_qmc_scenarios(s, N, sv, shift, True, True),
                lambda s: _hip.heston_qmc_scenarios(s, N, sv, shift, False, False)):
        first = run(base)
        clean = [(st.sum, st.sumsq, st.price, st.std_error) for st in first]
        assert all(math.isfinite(v) for row in clean for v in row)
        for field in (0, 1, 2, 3, 4, 6, 7, 8, 10):                                  # S K T r q, then the model but rho (refused: below)
            poisoned = list(base)
            poisoned[1] = (*base[1][:field], nan, *base[1][field + 1:])
            got = run(poisoned)
            assert math.isnan(got[1].price) and math.isnan(got[1].std_error) and math.isnan(got[1].sum) and got[1].n == first[1].n, field
            assert [(st.sum, st.sumsq, st.price, st.std_error) for i, st in enumerate(got) if i != 1] == clean[:1] + clean[2:], field
    with pytest.raises(ol.AccelerationError, match="rho must be in"):                # a NaN rho is no rho in [-1, 1]: refused, as olmc_heston refuses it
        _hip.heston_scenarios([base[0], (*base[1][:9], nan, base[1][10])], N, n, seed)
    # a negative spot answers NaN as everywhere else (poisoned()); v0 < 0 is a scenario like any other (ties above)
    got = _hip.heston_scenarios([base[0], scenario(S_=-1.0)], N, n, seed)
    assert math.isnan(got[1].price) and got[0].price == _hip.heston_scenarios([base[0]], N, n, seed)[0].price


# ------------------------------------------------------------------------------------ 11. the reference at workload level ----
def test_greeks_agree_with_the_reference_at_workload_level():
    """compute_greeks_unified of the reference over its own price_monte_carlo with v0 = sigma^2 (tests/golden/make_heston_greeks.py): for
    each of the nine Greeks the mean over 16 seeds within 5 combined standard errors of the device's 16-seed mean, once on Philox seeds
    and once on Sobol scrambles.  Same scheme, same n_steps: Euler's bias cancels.  Five, not the surface test's four: a scatter
    estimated from 16 runs is itself uncertain by about a fifth.  The seeds are fixed, so the outcome is deterministic."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heston_greeks.json")) as f:
        doc = json.load(f)
    inp = doc["inputs"]
    n = inp["n_steps"]
    assert len(doc["greeks"]) == 4 and len(inp["numpy_seeds"]) == 16
    for kw in (dict(n_paths=inp["n_paths"]), dict(n_paths=1 << 14, method="qmc")):
        for row in doc["greeks"]:
            p = pricer(tuple(doc["models"][row["model"]]))
            runs = np.asarray([[float(v) for v in ol.greeks_heston_monte_carlo(p, inp["S"], inp["K"], inp["T"], inp["r"], row["sigma"],
                                                                               row["option_type"], inp["q"], n_steps=n, seed=900 + s, **kw).values()]
                               for s in range(16)])
            assert runs.shape == (16, 9)
            for j, name in enumerate(GREEK_NAMES):
                mean, err = float(np.mean(runs[:, j])), float(np.std(runs[:, j], ddof=1) / 4.0)
                bound = 5.0 * math.hypot(err, row[name]["std_error"])
                print(kw.get("method", "pseudo"), row["model"], row["option_type"], name, mean, row[name]["mean"],
                      "distance / bound", abs(mean - row[name]["mean"]) / bound)
                assert abs(mean - row[name]["mean"]) <= bound, (kw, row["model"], row["option_type"], name, mean, err, row[name])
