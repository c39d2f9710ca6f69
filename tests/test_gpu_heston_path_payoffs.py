"""Asian, barrier and lookback options under Heston (HestonPricer.price_asian / price_barrier / price_lookback), one launch each.

The payoff of path i is pinned as what the reference's AsianOption / BarrierOption / LookbackOption.price computes from row i of
simulate_paths' spot matrix (tests/heston_path_oracle.py applies oracle/numpy_reference.py's restatements as they are).  So:
  1. Philox: the sums of the fused kernel against NumPy payoffs of the DEVICE's own matrix, which carries the same hardware normals
     (the CPU same-stream checker's software normals differ by 1e-7 and paths near the truncation part for good:
     test_gpu_property.py::test_path_matrices).  Bar rel 1e-10 / abs 1e-12, the project's bar for per-path ties.
  2. Philox, mirror leg: the normals recovered from the device's states under a model whose variance stays off 0, the literal recursion
     on their negatives.  The recovery reproduces the mirror spot to 6e-14 relative and the payoff sums to 3e-14 (CPU, known normals,
     4096 x 1024): the bar rel 1e-10 has a 3000x margin.
  3. Sobol: a NumPy oracle built from SciPy's points (per path, both constructions, both legs), over the full cross of n in
     {1, 2, 13, 64, 252}, the two models and N in {1, 1000, 2^12}, plus n = 1024 (the bridge's cap) and n = 4096 (sequential) once each.
  4. Agreement with price_monte_carlo and simulate_paths;  5. shards, determinism, the old entry points' bits;  6. the reference itself
     at workload level (tests/golden/heston_path_payoffs.json).
Barriers are discontinuous, so every tie first asserts that no path of its oracle matrix has its maximum or minimum within 1e-9
relative of the barrier (on the CPU the closest approach over N <= 4096, n <= 1024 was 9e-8; rounding differences are 1e-13).  No path
is left out: a seed that breaks the precondition is to be changed, not the rule.
"""
import functools
import json
import math
import os

import numpy as np
import pytest

from optionslab_amd import _hip
from optionslab_amd.monte_carlo import sobol_tables
from tests import heston_path_oracle as hpo
from tests import gpu_support
from tests.gpu_support import heston_pricer as pricer
from tests.heston_path_oracle import CALM, FELLER_VIOLATING, K, PAYOFFS, Q, R, S, T, USUAL

pytestmark = pytest.mark.gpu

TIE = dict(rel=1e-10, abs=1e-12)
STEPS = (1, 2, 13, 64, 252)
OPTION_TYPES = ("call", "put")


def assert_clear_of_the_barriers(spot, label):
    gap = hpo.barrier_clearance(spot)
    print(label, "closest approach to a barrier", gap)
    assert gap > 1e-9, (label, gap)


def philox_stats(model, family, kind, option_type, N, n, seed, antithetic=False, path_offset=0):
    payoff, barrier = hpo.payoff_code(family, kind)
    return _hip.heston_path_payoff(S, K, T, R, Q, option_type == "call", *model, payoff, barrier, N, n, seed, antithetic, path_offset)


def sobol_stats(model, family, kind, option_type, N, n, seed, construction, antithetic=False, point_offset=0):
    payoff, barrier = hpo.payoff_code(family, kind)
    sv, shift = sobol_tables(2 * n, seed, point_offset + N)
    return _hip.heston_qmc_path_payoff(S, K, T, R, Q, option_type == "call", *model, payoff, barrier, N, sv, shift, construction == "bridge",
                                       antithetic, point_offset)


check_sums = functools.partial(gpu_support.check_sums, tie=TIE)


# ------------------------------------------------------------------------------ 1. Philox: tie to the device's own matrix ----
@pytest.mark.parametrize("n", STEPS)
def test_philox_sums_match_the_payoffs_of_the_devices_own_path_matrix(n):
    for mi, model in enumerate((USUAL, FELLER_VIOLATING)):
        p = pricer(model)
        for N in (1, 63, 65, 1000, 4097):
            seed = 100 * n + N + mi
            spot, _var = p.simulate_paths(S, T, R, Q, N, n, seed)
            assert_clear_of_the_barriers(spot, (n, N, seed))
            for name, family, kind in PAYOFFS:
                for option_type in OPTION_TYPES:
                    check_sums(philox_stats(model, family, kind, option_type, N, n, seed), hpo.payoffs(spot, family, kind, option_type),
                               (mi, n, N, name, option_type))


def test_a_negative_start_variance_and_nan_inputs_at_the_c_abi():
    """v0 < 0 means what it means in olmc_heston (the first step is deterministic); a NaN input, the barrier's included, answers NaN."""
    model, N, n, seed = (2.0, 0.04, 0.3, -0.7, -0.01), 1000, 13, 3
    spot, var = _hip.heston_paths(S, T, R, Q, *model, N, n, seed, path_major=True)
    assert np.all(var[:, 0] == -0.01) and np.all(spot[:, 1] == spot[0, 1])
    assert_clear_of_the_barriers(spot, "v0 < 0")
    sv, shift = sobol_tables(2 * n, seed, N)
    for name, family, kind in PAYOFFS:
        check_sums(philox_stats(model, family, kind, "call", N, n, seed), hpo.payoffs(spot, family, kind, "call"), ("v0 < 0", name))
    for construction in ("bridge", "sequential"):
        qspot, _ = _hip.heston_qmc_paths(S, T, R, Q, *model, N, sv, shift, construction == "bridge", path_major=True)
        assert_clear_of_the_barriers(qspot, "v0 < 0 " + construction)
        for name, family, kind in PAYOFFS:
            check_sums(sobol_stats(model, family, kind, "put", N, n, seed, construction), hpo.payoffs(qspot, family, kind, "put"),
                       ("v0 < 0", construction, name))
    nan = float("nan")
    up_out = _hip.BARRIER_KINDS["up-and-out"]
    assert math.isnan(_hip.heston_path_payoff(S, K, T, R, Q, True, *USUAL, up_out, nan, N, n, seed).price)
    assert math.isnan(_hip.heston_path_payoff(S, K, T, nan, Q, True, *USUAL, _hip.PATH_ASIAN_ARITHMETIC, 0.0, N, n, seed).price)
    assert math.isnan(_hip.heston_qmc_path_payoff(S, K, T, R, Q, True, *USUAL, up_out, nan, N, sv, shift).price)
    assert math.isfinite(_hip.heston_path_payoff(S, K, T, R, Q, True, *USUAL, _hip.LOOKBACK_FIXED, nan, N, n, seed).price)   # ignored there


def test_a_barrier_met_at_date_0_is_decided_by_the_plain_comparison():
    """Date 0 is S itself: S >= barrier (up) / S <= barrier (down), also where the level IS the spot or one ulp from it."""
    N, n, seed = 1000, 13, 5
    euro = _hip.heston(S, K, T, R, Q, True, *USUAL, N, n, seed, False).sum
    below, above = math.nextafter(S, 0.0), math.nextafter(S, math.inf)
    spot, _ = pricer(USUAL).simulate_paths(S, T, R, Q, N, n, seed)
    for kind, level in (("up-and-out", S), ("up-and-out", below), ("down-and-out", S), ("down-and-out", above), ("up-and-in", S),
                        ("down-and-in", above)):                                   # all met at date 0
        got = _hip.heston_path_payoff(S, K, T, R, Q, True, *USUAL, _hip.BARRIER_KINDS[kind], level, N, n, seed).sum
        assert got == (0.0 if kind.endswith("out") else pytest.approx(euro, rel=1e-12)), (kind, level, got)
    # one ulp on the other side: date 0 does not cross, and the later dates decide as the matrix does
    # (a put under the up barrier, a call over the down one: the paths that stay on the spot's side of the level and pay)
    for kind, level, option_type in (("up-and-out", above, "put"), ("down-and-out", below, "call")):
        x = hpo.orc.barrier_from_paths(spot, K, T, R, level, kind, option_type, return_payoffs=True)[1]
        got = _hip.heston_path_payoff(S, K, T, R, Q, option_type == "call", *USUAL, _hip.BARRIER_KINDS[kind], level, N, n, seed)
        assert 0.0 < float(np.sum(x)) and got.sum == pytest.approx(float(np.sum(x)), **TIE), (kind, level)


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
    print((N, n), "min variance", float(var.min()), "mirror", float(mirror_var.min()))
    assert float(mirror_var.min()) > 0.0
    assert_clear_of_the_barriers(spot, (N, n, "leg 0"))
    assert_clear_of_the_barriers(mirror, (N, n, "mirror"))
    for name, family, kind in PAYOFFS:
        for option_type in OPTION_TYPES:
            plain = philox_stats(CALM, family, kind, option_type, N, n, seed, antithetic=False)
            both = philox_stats(CALM, family, kind, option_type, N, n, seed, antithetic=True)
            x = hpo.payoffs(mirror, family, kind, option_type)
            print((N, n), name, option_type, "mirror sum", both.sum - plain.sum, "oracle", float(np.sum(x)))
            assert plain.n == N and both.n == 2 * N
            assert both.sum - plain.sum == pytest.approx(float(np.sum(x)), rel=1e-10), (name, option_type)
            assert both.sumsq - plain.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10), (name, option_type)


# ----------------------------------------------------------------------------------- 3. Sobol: per-path tie to the oracle ----
SOBOL_COUNTS = (1, 1000, 1 << 12)
SOBOL_CASES = [(n, mi, N, ("bridge", "sequential")) for n in STEPS for mi in (0, 1) for N in SOBOL_COUNTS]      # the full cross
SOBOL_CASES += [(1024, 0, 1000, ("bridge", "sequential")), (4096, 1, 1000, ("sequential",))]      # once each: the bridge's cap; beyond it


@pytest.mark.parametrize("n,mi,N,constructions", SOBOL_CASES, ids=[f"n{c[0]}-model{c[1]}-N{c[2]}" for c in SOBOL_CASES])
def test_sobol_sums_match_the_numpy_oracle(n, mi, N, constructions):
    model = (USUAL, FELLER_VIOLATING)[mi]
    seed = 1000 + n + mi
    spots = hpo.sobol_spots(n, N, seed, model, constructions)
    for construction in constructions:
        for leg in (0, 1):
            assert_clear_of_the_barriers(spots[(construction, leg)], (n, N, construction, leg))
        for name, family, kind in PAYOFFS:
            for option_type in OPTION_TYPES:
                x0, x1 = (hpo.payoffs(spots[(construction, leg)], family, kind, option_type) for leg in (0, 1))
                for antithetic, x in ((False, x0), (True, np.concatenate([x0, x1]))):
                    check_sums(sobol_stats(model, family, kind, option_type, N, n, seed, construction, antithetic), x,
                               (n, N, mi, construction, name, option_type, antithetic))


# ------------------------------------------------------------------------------------- 4. agreement with the neighbours ----
@pytest.mark.parametrize("kw", [dict(), dict(method="qmc"), dict(method="qmc", path_construction="sequential")],
                         ids=["pseudo", "bridge", "sequential"])
def test_the_price_is_the_discounted_mean_payoff_of_simulate_paths(kw):
    N, n, seed = 4097, 64, 21
    disc = math.exp(-R * T)
    for model in (USUAL, FELLER_VIOLATING):
        p = pricer(model)
        spot, _var = p.simulate_paths(S, T, R, Q, N, n, seed, **kw)
        assert_clear_of_the_barriers(spot, (kw, model))
        for name, family, kind in PAYOFFS:
            for option_type in OPTION_TYPES:
                x = hpo.payoffs(spot, family, kind, option_type)
                price = hpo.price_method(p, family, kind, option_type, n_paths=N, n_steps=n, seed=seed, **kw)
                assert isinstance(price, np.float64)
                assert float(price) == pytest.approx(disc * float(np.mean(x)), rel=1e-10), (name, option_type)
                price2, err = hpo.price_method(p, family, kind, option_type, n_paths=N, n_steps=n, seed=seed, return_error=True, **kw)
                assert price2 == price and isinstance(err, float)
                assert err == pytest.approx(disc * float(np.std(x)) / math.sqrt(N), rel=1e-6), (name, option_type)


def test_knock_out_plus_knock_in_is_the_european_and_the_payoffs_are_ordered():
    N, n, seed = 1 << 14, 64, 33
    sv, shift = sobol_tables(2 * n, seed, N)
    kinds = _hip.BARRIER_KINDS
    for is_call in (True, False):
        runs = [(_hip.heston(S, K, T, R, Q, is_call, *USUAL, N, n, seed, False),
                 lambda payoff, b: _hip.heston_path_payoff(S, K, T, R, Q, is_call, *USUAL, payoff, b, N, n, seed))]
        for bridge in (True, False):
            runs.append((_hip.heston_qmc(S, K, T, R, Q, is_call, *USUAL, N, sv, shift, bridge),
                         lambda payoff, b, bridge=bridge: _hip.heston_qmc_path_payoff(S, K, T, R, Q, is_call, *USUAL, payoff, b, N, sv, shift, bridge)))
        for euro, call in runs:
            for side, level in (("up", hpo.UP), ("down", hpo.DOWN)):
                out, inn = call(kinds[side + "-and-out"], level), call(kinds[side + "-and-in"], level)
                assert out.sum > 0.0 and inn.sum > 0.0
                assert out.sum + inn.sum == pytest.approx(euro.sum, rel=1e-12), (is_call, side)
            if is_call:
                assert call(_hip.LOOKBACK_FIXED, 0.0).price >= euro.price
                assert call(_hip.PATH_ASIAN_GEOMETRIC, 0.0).price <= call(_hip.PATH_ASIAN_ARITHMETIC, 0.0).price


def test_with_profiling_on_the_launch_counts_once_in_the_kernel_time():
    N, n = 1000, 64
    sv, shift = sobol_tables(2 * n, 1, N)
    calls = [lambda: _hip.heston_path_payoff(S, K, T, R, Q, True, *USUAL, _hip.PATH_ASIAN_ARITHMETIC, 0.0, N, n, 1, True)]
    for bridge in (True, False):
        calls.append(lambda b=bridge: _hip.heston_qmc_path_payoff(S, K, T, R, Q, True, *USUAL, _hip.LOOKBACK_FLOATING, 0.0, N, sv, shift, b, True))
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


# --------------------------------------------------------------------------------------------- 5. shards and determinism ----
def test_shards_of_one_stream_or_sequence_add_up():
    N, n, a, seed = 4097, 64, 1000, 9                                              # a is no multiple of 64
    for model, option_type, antithetic in ((USUAL, "call", False), (FELLER_VIOLATING, "put", True)):
        for name, family, kind in PAYOFFS:
            calls = [lambda off, cnt: philox_stats(model, family, kind, option_type, cnt, n, seed, antithetic, off)]
            for construction in ("bridge", "sequential"):
                calls.append(lambda off, cnt, c=construction: sobol_stats(model, family, kind, option_type, cnt, n, seed, c, antithetic, off))
            for call in calls:
                whole, lo, hi = call(0, N), call(0, a), call(a, N - a)
                assert whole.n == lo.n + hi.n == N * (2 if antithetic else 1)
                assert whole.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12), name
                assert whole.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12), name


def test_equal_seeds_give_equal_bits():
    p = pricer(USUAL)
    for kw in (dict(), dict(method="qmc"), dict(method="qmc", path_construction="sequential")):
        for name, family, kind in PAYOFFS:
            price = lambda seed, n=64: hpo.price_method(p, family, kind, "call", n_paths=4097, n_steps=n, seed=seed, antithetic=True, **kw)
            first, other = price(11), price(12)
            price(12, 100)                                                          # other tables, another plan, other slabs in between
            assert price(11) == first and price(12) == other and first != other, (kw, name)


# Captured on the commit before these kernels existed (same device kind): HestonPricer(*USUAL), S K T r q as above.
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
    N, n, seed = 4097, 64, 77
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


# ------------------------------------------------------------------------------------- 6. the reference at workload level ----
def test_prices_agree_with_the_reference_at_workload_level():
    """The reference's three option classes on the reference HestonPricer's own matrix (N = 100 000 x 64, a NumPy seed): each price
    within 4 combined standard errors.  64 comparisons at four standard errors raise a false alarm about 0.4 % of the time for a fresh
    seed; the seeds are fixed, so the outcome is deterministic thereafter."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heston_path_payoffs.json")) as f:
        doc = json.load(f)
    models = {k: tuple(v) for k, v in doc["models"].items()}
    n = doc["inputs"]["n_steps"]
    by_name = {name: (family, kind) for name, family, kind in PAYOFFS}
    for kw in (dict(n_paths=200_000, seed=2024), dict(n_paths=1 << 14, seed=2024, method="qmc")):
        for row in doc["prices"]:
            family, kind = by_name[row["payoff"]]
            price, err = hpo.price_method(pricer(models[row["model"]]), family, kind, row["option_type"], n_steps=n, return_error=True, **kw)
            bound = 4.0 * math.hypot(err, row["std_error"])
            print(kw.get("method", "pseudo"), row["model"], row["payoff"], row["option_type"], float(price), row["price"],
                  "distance / bound", abs(float(price) - row["price"]) / bound)
            assert abs(float(price) - row["price"]) <= bound, (kw, row, float(price), err)
