"""Path-dependent payoffs, the surface, the autocallable and the cliquet on Merton / Kou jump-diffusion paths (include/olmc_jump.h).

Leg 0 of every oljd_* entry point is tied to the payoffs oracle/numpy_reference.py computes from the device's OWN path matrix
(olmc_jump_paths, a kernel from before these entry points), the mirror leg to a matrix recovered from two olmc_jump_paths runs (at sigma
and at sigma = 0: their difference isolates the jump sums), and the antithetic sums to the payoffs of both matrices.  Bars: TIE for
sums against per-path payoffs, rel 1e-12 for shards, 3.5 standard errors against a closed form and 4 combined standard errors between
two Monte Carlo prices.  Every tie first asserts that no path comes within 1e-9 (relative) of a level it could cross: the kernels
decide in log space, the matrix route after an exponential.
The device's own matrix (olmc_jump_paths, and oljd_paths with both legs) is pinned in tests/test_gpu_path_matrices_exact.py: to a
long-double recursion on the stream's draws, the jump counts to SciPy's Poisson quantile.
"""
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import heston_path_oracle as hpo
from tests import gpu_support
from tests.test_gpu_heston_structured import (AUTOCALL, CLIQUET, COUNTS, SHAPES, assert_clear_of_the_levels, autocall_payoffs, branch_mix,
                                               cliquet_payoffs)

pytestmark = pytest.mark.gpu

S, K, T, R, Q, UP, DOWN, PAYOFFS = hpo.S, hpo.K, hpo.T, hpo.R, hpo.Q, hpo.UP, hpo.DOWN, hpo.PAYOFFS
SIGMA = 0.2
TIE = dict(rel=1e-10, abs=1e-12)
EUROPEAN = _hip.JD_EUROPEAN
# (kou, lambda_j, a1, a2, a3): M0, M1 (multi-jump steps), K0, K1
MODELS = ((False, 0.5, -0.1, 0.2, 0.0), (False, 40.0, 0.02, 0.1, 0.0), (True, 1.0, 0.4, 10.0, 5.0), (True, 60.0, 0.6, 25.0, 20.0))
M0, M1, K0, K1 = MODELS
NAMES = ("M0", "M1", "K0", "K1")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jump_parent_bits.json")


def too_intense(model, n):
    """More than 20 expected jumps per step: refused by every jump entry point (K1 at n <= 2)."""
    return model[1] * T / n > 20.0


def matrix(model, N, n, seed, sigma=SIGMA):
    return _hip.jump_paths(S, T, R, sigma, Q, *model, N, n, seed, path_major=True)


def mirror_matrix(model, N, n, seed):
    return _hip.jd_paths(S, T, R, SIGMA, Q, model, N, n, seed, mirror=True, path_major=True)


def price(model, family, kind, option_type, N, n, seed, antithetic=False, path_offset=0):
    payoff, level = hpo.payoff_code(family, kind)
    return _hip.jd_price(S, K, T, R, SIGMA, Q, option_type == "call", model, payoff, level, N, n, seed, antithetic, path_offset)


def european(model, option_type, N, n, seed, antithetic=False, path_offset=0, strike=K, sigma=SIGMA):
    return _hip.jd_price(S, strike, T, R, sigma, Q, option_type == "call", model, EUROPEAN, 0.0, N, n, seed, antithetic, path_offset)


def european_payoffs(spot, option_type, strike=K, column=-1):
    sign = 1.0 if option_type == "call" else -1.0
    return np.maximum(sign * (spot[:, column] - strike), 0.0)


def assert_clear_of_the_barriers(spot, label):
    gap = hpo.barrier_clearance(spot)
    assert gap > 1e-9, (label, gap)


check_sums = functools.partial(gpu_support.check_sums, tie=TIE)


def check_every_payoff(label, spots, model, N, n, seed, antithetic):
    """The eight payoffs and the European, call and put, against the legs' matrices in the order the sums take them."""
    for leg, spot in enumerate(spots):
        assert_clear_of_the_barriers(spot, (label, "leg", leg))
    for option_type in ("call", "put"):
        for name, family, kind in PAYOFFS:
            x = np.concatenate([hpo.payoffs(spot, family, kind, option_type) for spot in spots])
            check_sums(price(model, family, kind, option_type, N, n, seed, antithetic), x, (label, name, option_type))
        x = np.concatenate([european_payoffs(spot, option_type) for spot in spots])
        check_sums(european(model, option_type, N, n, seed, antithetic), x, (label, "european", option_type))


# ------------------------------------------------------------------------------------ 1. leg 0: the device's own matrix ----
@pytest.mark.parametrize("n", (1, 2, 13, 64, 252))
def test_leg_0_sums_match_the_payoffs_of_the_devices_own_path_matrix(n):
    for mi, model in enumerate(MODELS):
        if too_intense(model, n):
            with pytest.raises(AccelerationError, match="must be <= 20 jumps per step"):
                european(model, "call", 63, n, 1)
            continue
        for N in (1, 63, 65, 1000, 4097):
            seed = 100 * n + N + mi
            spot = matrix(model, N, n, seed)
            label = (NAMES[mi], n, N, seed)
            check_every_payoff(label, [spot], model, N, n, seed, False)
            for option_type in ("call", "put"):
                old = _hip.jump_diffusion(S, K, T, R, SIGMA, Q, option_type == "call", *model, N, n, seed)
                new = european(model, option_type, N, n, seed)
                assert new.n == old.n and new.sum == pytest.approx(old.sum, **TIE) and new.sumsq == pytest.approx(old.sumsq, **TIE), label


def test_the_public_methods_return_the_discounted_mean_and_its_standard_error():
    N, n, seed = 1000, 13, 21
    disc = math.exp(-R * T)
    for model, p in ((M0, ol.MertonJumpDiffusion(*M0[1:4])), (K0, ol.KouJumpDiffusion(*K0[1:]))):
        spot = matrix(model, N, n, seed)
        assert np.array_equal(spot, p.simulate_paths(S, T, R, SIGMA, Q, N, n, seed))
        assert np.array_equal(mirror_matrix(model, N, n, seed), p.simulate_paths(S, T, R, SIGMA, Q, N, n, seed, mirror=True))
        assert_clear_of_the_barriers(spot, "methods")
        got = {"asian": p.price_asian(S, K, T, R, SIGMA, Q, "put", "geometric", N, n, seed, False, True),
               "barrier": p.price_barrier(S, K, T, R, SIGMA, DOWN, Q, "call", "down-and-in", N, n, seed, False, True),
               "lookback": p.price_lookback(S, K, T, R, SIGMA, Q, "call", "fixed", N, n, seed, False, True)}
        want = {"asian": hpo.payoffs(spot, "asian", "geometric", "put"), "barrier": hpo.payoffs(spot, "barrier", "down-and-in", "call"),
                "lookback": hpo.payoffs(spot, "lookback", "fixed", "call")}
        for name, (value, error) in got.items():
            x = want[name]
            assert value == pytest.approx(disc * float(np.mean(x)), rel=1e-10), name
            assert error == pytest.approx(disc * float(np.std(x)) / math.sqrt(N), rel=1e-6), name
            assert isinstance(value, np.float64) and isinstance(error, float)
        assert_clear_of_the_levels(spot, 4, "methods")
        value = p.price_autocallable(S, T, R, SIGMA, Q, *AUTOCALL, 4, N, n, seed)
        assert value == pytest.approx(float(np.mean(autocall_payoffs(spot, 4))), rel=1e-10)
        value = p.price_cliquet(S, T, R, SIGMA, Q, *CLIQUET, 4, N, n, seed)
        assert value == pytest.approx(disc * float(np.mean(cliquet_payoffs(spot, 4))), rel=1e-10)
        # the surface: (strikes, maturities) -> [i, j], each cell discounted over its own maturity
        prices = p.price_surface(S, [95.0, 105.0], [T, 4 * T / n], R, SIGMA, Q, "call", N, n, seed)
        for i, strike in enumerate((95.0, 105.0)):
            for j, m in enumerate((n, 4)):
                want_cell = math.exp(-R * m * T / n) * float(np.mean(european_payoffs(spot, "call", strike, m)))
                assert prices[i, j] == pytest.approx(want_cell, rel=1e-10), (i, j)
        # price_monte_carlo: antithetic=False is the old launch, True the path and its mirror
        old = _hip.jump_diffusion(S, K, T, R, SIGMA, Q, True, *model, N, n, seed)
        assert p.price_monte_carlo(S, K, T, R, SIGMA, "call", Q, N, n, seed) == old.price
        both = european(model, "call", N, n, seed, True)
        assert p.price_monte_carlo(S, K, T, R, SIGMA, "call", Q, N, n, seed, True, antithetic=True) == (both.price, both.std_error)


# ------------------------------------------------------------------------------------------------------- 2. the mirror ----
@pytest.mark.parametrize("N,n", [(257, 13), (4096, 64)])
def test_the_mirror_leg_negates_the_diffusion_and_shares_the_jumps(N, n):
    seed = 17 + n
    dt = T / n
    for mi, model in enumerate(MODELS):
        spot = matrix(model, N, n, seed)
        for path_major in (True, False):
            old = _hip.jump_paths(S, T, R, SIGMA, Q, *model, N, n, seed, path_major=path_major)
            new = _hip.jd_paths(S, T, R, SIGMA, Q, model, N, n, seed, mirror=False, path_major=path_major)
            assert np.array_equal(old.view(np.uint64), new.view(np.uint64)), (NAMES[mi], path_major)
        # the jump sum of every step from the device's own matrices: sigma = 0 leaves the compensated drift and the jumps
        kou, lam, a1, a2, a3 = model
        kappa = (a1 * a2 / (a2 - 1) + (1 - a1) * a3 / (a3 + 1) - 1) if kou else math.exp(a1 + 0.5 * a2 * a2) - 1
        jumps = np.diff(np.log(matrix(model, N, n, seed, sigma=0.0)), axis=1) - (R - Q - lam * kappa) * dt
        jumped = float(np.mean(np.abs(jumps) > 1e-12))
        print(NAMES[mi], "share of steps with a jump", jumped, "expected", 1 - math.exp(-lam * dt))
        assert jumped == pytest.approx(1 - math.exp(-lam * dt), abs=5 * math.sqrt(0.25 / (N * n)) + 1e-3)
        drift = (R - Q - lam * kappa - 0.5 * SIGMA * SIGMA) * dt
        want_log = math.log(S) + np.cumsum(2.0 * (drift + jumps) - np.diff(np.log(spot), axis=1), axis=1)
        mirror = mirror_matrix(model, N, n, seed)
        assert np.all(mirror[:, 0] == S)
        worst = float(np.max(np.abs(mirror[:, 1:] / np.exp(want_log) - 1.0)))
        print(NAMES[mi], N, n, "mirror against the recovery: worst relative difference", worst)
        assert worst <= 1e-12, (NAMES[mi], worst)
        step_major = _hip.jd_paths(S, T, R, SIGMA, Q, model, N, n, seed, mirror=True, path_major=False)
        assert np.array_equal(step_major.T, mirror)
        # antithetic sums: both legs' payoffs, 2 N samples
        label = ("antithetic", NAMES[mi], N, n)
        check_every_payoff(label, [spot, mirror], model, N, n, seed, True)
        strikes, steps = [95.0, 105.0, K], [n, 4, n]
        for option_type in ("call", "put"):
            cells = _hip.jd_surface_prices(S, T, R, SIGMA, Q, option_type == "call", model, strikes, steps, N, n, seed, True)
            for st, strike, m in zip(cells, strikes, steps):
                check_sums(st, np.concatenate([european_payoffs(leg, option_type, strike, m) for leg in (spot, mirror)]), (label, "cell", strike, m))
        f, periods = (4, 4) if n == 13 else (21, 12)
        for leg in (spot, mirror):
            assert_clear_of_the_levels(leg, f, label)
        check_sums(_hip.jd_autocallable(S, T, R, SIGMA, Q, model, *AUTOCALL, f, N, n, seed, True),
                   np.concatenate([autocall_payoffs(leg, f) for leg in (spot, mirror)]), (label, "autocallable"))
        check_sums(_hip.jd_cliquet(S, T, R, SIGMA, Q, model, *CLIQUET, periods, N, n, seed, True),
                   np.concatenate([cliquet_payoffs(leg, periods) for leg in (spot, mirror)]), (label, "cliquet"))


# ------------------------------------------------------------------------------------------- 3. date 0 and identities ----
def test_a_barrier_met_at_date_0_is_decided_by_the_plain_comparison():
    """Date 0 is S itself: S >= barrier (up) / S <= barrier (down), also where the level IS the spot or one ulp from it."""
    N, n, seed = 1000, 13, 5
    for model in (M0, K1):
        euro = european(model, "call", N, n, seed).sum
        below, above = math.nextafter(S, 0.0), math.nextafter(S, math.inf)
        spot = matrix(model, N, n, seed)
        for kind, level in (("up-and-out", S), ("up-and-out", below), ("down-and-out", S), ("down-and-out", above), ("up-and-in", S),
                            ("down-and-in", above)):                                   # all met at date 0
            got = _hip.jd_price(S, K, T, R, SIGMA, Q, True, model, _hip.BARRIER_KINDS[kind], level, N, n, seed).sum
            assert got == (0.0 if kind.endswith("out") else pytest.approx(euro, rel=1e-12)), (kind, level, got)
        # one ulp on the other side: date 0 does not cross, and the later dates decide as the matrix does
        for kind, level, option_type in (("up-and-out", above, "put"), ("down-and-out", below, "call")):
            x = hpo.orc.barrier_from_paths(spot, K, T, R, level, kind, option_type, return_payoffs=True)[1]
            got = _hip.jd_price(S, K, T, R, SIGMA, Q, option_type == "call", model, _hip.BARRIER_KINDS[kind], level, N, n, seed)
            assert 0.0 < float(np.sum(x)) and got.sum == pytest.approx(float(np.sum(x)), **TIE), (kind, level)


@pytest.mark.parametrize("antithetic", (False, True))
def test_knock_in_plus_knock_out_is_the_european(antithetic):
    N, n, seed = 4097, 13, 23
    for model in MODELS:
        for option_type in ("call", "put"):
            euro = european(model, option_type, N, n, seed, antithetic).sum
            for side in ("up", "down"):
                parts = [price(model, "barrier", f"{side}-and-{way}", option_type, N, n, seed, antithetic).sum for way in ("in", "out")]
                assert parts[0] + parts[1] == pytest.approx(euro, rel=1e-12), (model, option_type, side)


# ----------------------------------------------------------------------------------------------------------- 4. surface ----
@pytest.mark.parametrize("n", (13, 64))
def test_surface_cells_are_the_columns_of_the_matrix(n):
    N = 1000
    cell_sets = {1: ([K], [n]), 3: ([95.0, 105.0, K], [n, 1, n]),
                 16: ([80.0 + 3.0 * i for i in range(15)] + [K], [1, n, 5, 5, 5, 2, n, 1, 7, 7, n - 1, 3, 3, 3, n, n])}
    for mi, model in enumerate(MODELS):
        seed = 40 + n + mi
        legs = [matrix(model, N, n, seed), mirror_matrix(model, N, n, seed)]
        for k, (strikes, steps) in cell_sets.items():
            for antithetic in (False, True):
                spots = legs if antithetic else legs[:1]
                for option_type in ("call", "put"):
                    cells = _hip.jd_surface_prices(S, T, R, SIGMA, Q, option_type == "call", model, strikes, steps, N, n, seed, antithetic)
                    assert len(cells) == k
                    for st, strike, m in zip(cells, strikes, steps):
                        x = np.concatenate([european_payoffs(spot, option_type, strike, m) for spot in spots])
                        check_sums(st, x, (NAMES[mi], k, strike, m, option_type, antithetic))
                        disc = math.exp(-R * m * T / n)
                        assert st.price == pytest.approx(disc * float(np.mean(x)), rel=1e-10)
                    euro = european(model, option_type, N, n, seed, antithetic)
                    assert cells[-1].sum == pytest.approx(euro.sum, **TIE) and cells[-1].sumsq == pytest.approx(euro.sumsq, **TIE)


# ---------------------------------------------------------------------------------------------------------- 5. products ----
@pytest.mark.parametrize("n,f,periods", SHAPES, ids=["n%d-f%d-p%d" % s for s in SHAPES])
def test_product_sums_match_the_payoffs_of_the_devices_own_path_matrix(n, f, periods):
    for mi, model in enumerate(MODELS):
        if too_intense(model, n):
            continue
        for N in COUNTS:
            seed = 1000 * n + N + mi
            spot = matrix(model, N, n, seed)
            label = (NAMES[mi], n, f, periods, N, seed)
            assert_clear_of_the_levels(spot, f, label)
            check_sums(_hip.jd_autocallable(S, T, R, SIGMA, Q, model, *AUTOCALL, f, N, n, seed), autocall_payoffs(spot, f), (label, "autocallable"))
            x = cliquet_payoffs(spot, periods)
            check_sums(_hip.jd_cliquet(S, T, R, SIGMA, Q, model, *CLIQUET, periods, N, n, seed), x, (label, "cliquet"))
            if N == 4097 and n == 64:
                early, coupon, loss = branch_mix(spot, f)
                zero = float(np.mean(x == 0.0))
                print(label, "early", early, "coupon", coupon, "loss", loss, "zero-payoff cliquets", zero)
                assert early > 0.3 and loss > 0.05 and 0.1 < zero < 0.9                 # every branch of the payoffs is exercised


# ------------------------------------------------------------------------------- 6. shards, determinism, offsets ----
def stats_calls(model, n, f, periods, seed, antithetic):
    """{label: call(count, offset)} over every reducing entry point."""
    calls = {name + "-" + ot: (lambda c, o, fam=family, kind=kind, ot=ot: price(model, fam, kind, ot, c, n, seed, antithetic, o))
             for name, family, kind in PAYOFFS for ot in ("call", "put")}
    calls["european"] = lambda c, o: european(model, "call", c, n, seed, antithetic, o)
    calls["autocallable"] = lambda c, o: _hip.jd_autocallable(S, T, R, SIGMA, Q, model, *AUTOCALL, f, c, n, seed, antithetic, o)
    calls["cliquet"] = lambda c, o: _hip.jd_cliquet(S, T, R, SIGMA, Q, model, *CLIQUET, periods, c, n, seed, antithetic, o)
    for i in range(3):
        calls[f"cell{i}"] = lambda c, o, i=i: _hip.jd_surface_prices(S, T, R, SIGMA, Q, True, model, [95.0, 105.0, K], [n, 4, n], c, n, seed,
                                                                    antithetic, o)[i]
    return calls


@pytest.mark.parametrize("antithetic", (False, True))
def test_uneven_shards_add_up_to_the_whole(antithetic):
    N, n, f, periods, seed = 4133, 13, 4, 4, 9
    for model in (M1, K0):
        for label, call in stats_calls(model, n, f, periods, seed, antithetic).items():
            whole = call(N, 0)
            for cuts in ((1000,), (63, 2001)):                                          # no cut is a multiple of 64
                edges = (0,) + cuts + (N,)
                parts = [call(b - a, a) for a, b in zip(edges, edges[1:])]
                assert whole.n == sum(p.n for p in parts) == N * (2 if antithetic else 1), label
                assert whole.sum == pytest.approx(sum(p.sum for p in parts), rel=1e-12), label
                assert whole.sumsq == pytest.approx(sum(p.sumsq for p in parts), rel=1e-12), label
            combined = _hip.combine_stats([(p.sum, p.sumsq, p.n) for p in parts], R, T)
            if label in ("european", "cliquet") or label.startswith(("asian", "barrier", "lookback")):
                assert combined.price == pytest.approx(whole.price, rel=1e-12), label


def test_equal_arguments_give_equal_words():
    from tests import call_catalogue as cc

    N, n = 4133, 13
    for model in (M1, K1):
        first = {label: cc.words(call(N, 0)) for label, call in stats_calls(model, n, 4, 4, 11, True).items()}
        other = {label: cc.words(call(N, 0)) for label, call in stats_calls(model, n, 4, 4, 12, True).items()}
        again = {label: cc.words(call(N, 0)) for label, call in stats_calls(model, n, 4, 4, 11, True).items()}
        for label in first:
            assert np.array_equal(first[label], again[label]), label
            assert not np.array_equal(first[label], other[label]), label


def test_a_path_offset_beyond_2_to_the_32_names_olmc_jump_diffusions_paths():
    N, n, seed, offset = 1000, 12, 3, (1 << 32) + 5
    for model in (M1, K0):
        for option_type in ("call", "put"):
            old = _hip.jump_diffusion(S, K, T, R, SIGMA, Q, option_type == "call", *model, N, n, seed, path_offset=offset)
            new = european(model, option_type, N, n, seed, False, offset)
            assert new.sum == pytest.approx(old.sum, **TIE) and new.sumsq == pytest.approx(old.sumsq, **TIE)
            assert new.sum != european(model, option_type, N, n, seed, False, 5).sum             # the high word of the path index is read
        # the matrix names paths [0, N): a launch that ends at N ties to its last rows, and shards across 2^32 add up to the launch
        spot = matrix(model, N, n, seed)
        assert_clear_of_the_barriers(spot, "offset")
        tail = price(model, "barrier", "up-and-out", "call", 300, n, seed, False, N - 300)
        check_sums(tail, hpo.payoffs(spot[N - 300:], "barrier", "up-and-out", "call"), "the last 300 rows")
        lo = (1 << 32) - 300
        for label, call in stats_calls(model, n, 3, 12, seed, True).items():
            whole, a, b = call(N, lo), call(300, lo), call(N - 300, 1 << 32)
            assert whole.sum == pytest.approx(a.sum + b.sum, rel=1e-12) and whole.sumsq == pytest.approx(a.sumsq + b.sumsq, rel=1e-12), label


def test_more_than_one_grid_stride_trip():
    N, n, seed = 70_001, 13, 31
    for model in (M1, K0):
        spot = matrix(model, N, n, seed)
        mirror = mirror_matrix(model, N, n, seed)
        for leg in (spot, mirror):
            assert_clear_of_the_barriers(leg, "70001")
            assert_clear_of_the_levels(leg, 4, "70001")
        check_sums(price(model, "barrier", "down-and-in", "put", N, n, seed, True),
                   np.concatenate([hpo.payoffs(leg, "barrier", "down-and-in", "put") for leg in (spot, mirror)]), "barrier")
        check_sums(price(model, "asian", "arithmetic", "call", N, n, seed), hpo.payoffs(spot, "asian", "arithmetic", "call"), "asian")
        check_sums(_hip.jd_autocallable(S, T, R, SIGMA, Q, model, *AUTOCALL, 4, N, n, seed, True),
                   np.concatenate([autocall_payoffs(leg, 4) for leg in (spot, mirror)]), "autocallable")
        check_sums(_hip.jd_cliquet(S, T, R, SIGMA, Q, model, *CLIQUET, 4, N, n, seed), cliquet_payoffs(spot, 4), "cliquet")
        cell = _hip.jd_surface_prices(S, T, R, SIGMA, Q, False, model, [K], [7], N, n, seed, True)[0]
        check_sums(cell, np.concatenate([european_payoffs(leg, "put", K, 7) for leg in (spot, mirror)]), "cell")


# ------------------------------------------------------------------------------------------------ 7. statistical anchors ----
ANCHOR_N, ANCHOR_STEPS, ANCHOR_SEED = 1 << 16, 32, 8         # fixed before the first run


def z_score(st, value):
    return (st.price - value) / st.std_error


@pytest.mark.parametrize("antithetic", (False, True))
def test_merton_europeans_agree_with_the_series(antithetic):
    p = ol.MertonJumpDiffusion(*M0[1:4])
    for option_type in ("call", "put"):
        st = european(M0, option_type, ANCHOR_N, ANCHOR_STEPS, ANCHOR_SEED, antithetic)
        z = z_score(st, p.price(S, K, T, R, SIGMA, option_type, Q))
        print("M0", option_type, "antithetic", antithetic, "price", st.price, "se", st.std_error, "z", z)
        assert st.n == ANCHOR_N * (2 if antithetic else 1) and abs(z) <= 3.5


@pytest.mark.parametrize("antithetic", (False, True))
def test_kou_paths_are_martingales(antithetic):
    for model in ((True, 3.0, 0.4, 10.0, 5.0), K1):
        st = european(model, "call", ANCHOR_N, ANCHOR_STEPS, ANCHOR_SEED, antithetic, strike=1e-6)
        z = z_score(st, S * math.exp(-Q * T) - 1e-6 * math.exp(-R * T))
        print(model, "antithetic", antithetic, "price", st.price, "se", st.std_error, "z", z)
        assert abs(z) <= 3.5
    # the mirror leg alone
    for model in ((True, 3.0, 0.4, 10.0, 5.0), K1):
        x = mirror_matrix(model, ANCHOR_N, ANCHOR_STEPS, ANCHOR_SEED)[:, -1]
        z = (float(np.mean(x)) - S * math.exp((R - Q) * T)) / (float(np.std(x)) / math.sqrt(ANCHOR_N))
        print(model, "mirror leg alone: z", z)
        assert abs(z) <= 3.5


@pytest.mark.parametrize("antithetic", (False, True))
def test_without_jumps_the_prices_are_the_gbm_kernels(antithetic):
    N, n, seed = ANCHOR_N, ANCHOR_STEPS, ANCHOR_SEED
    for model in ((False, 0.0, -0.1, 0.2, 0.0), (True, 0.0, 0.4, 10.0, 5.0)):
        for option_type in ("call", "put"):
            for name, family, kind in PAYOFFS:
                st = price(model, family, kind, option_type, N, n, seed, antithetic)
                if family == "asian":
                    ref = ol.AsianOption(S, K, T, R, SIGMA, Q, seed).price(N, n, kind, option_type, antithetic, True)
                elif family == "barrier":
                    ref = ol.BarrierOption(S, K, T, R, SIGMA, Q, seed, hpo.barrier_level(kind)).price(N, n, kind, option_type, antithetic, True)
                else:
                    ref = ol.LookbackOption(S, K, T, R, SIGMA, Q, seed).price(N, n, kind, option_type, antithetic, True)
                z = (st.price - float(ref[0])) / math.hypot(st.std_error, float(ref[1]))
                print(name, option_type, "antithetic", antithetic, "jump", st.price, "gbm", float(ref[0]), "z", z)
                assert abs(z) <= 4.0, (name, option_type, z)
            st = european(model, option_type, N, n, seed, antithetic)
            z = z_score(st, ol.black_scholes(S, K, T, R, SIGMA, option_type, Q))
            print("european", option_type, "antithetic", antithetic, "z", z)
            assert abs(z) <= 3.5


# ------------------------------------------------------------------------ 8. the old entry points keep their bits ----
def hex_words(a):
    return " ".join("%016x" % int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel())


def test_the_old_entry_points_give_the_bits_they_gave_before_this_header_existed():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert (doc["S"], doc["K"], doc["T"], doc["r"], doc["q"], doc["sigma"]) == (S, K, T, R, Q, SIGMA)
    seed = doc["seed"]
    assert len(doc["cases"]) == 12
    for case in doc["cases"]:
        model, N, n = MODELS[NAMES.index(case["model"])], case["n_paths"], case["n_steps"]
        label = (case["model"], N, n)
        if "refused_price" in case:
            for call in (lambda: _hip.jump_diffusion(S, K, T, R, SIGMA, Q, True, *model, N, n, seed), lambda: _hip.jump_paths(S, T, R, SIGMA, Q, *model, N, n, seed)):
                with pytest.raises(AccelerationError) as exc:
                    call()
                assert str(exc.value) == case["refused_price"], label
            continue
        for option_type in ("call", "put"):
            st = _hip.jump_diffusion(S, K, T, R, SIGMA, Q, option_type == "call", *model, N, n, seed)
            assert hex_words([st.sum, st.sumsq]) == case[option_type]["sums"] and st.n == case[option_type]["n"], (label, option_type)
        for layout in ("path_major", "step_major"):
            want = case[layout]
            m = _hip.jump_paths(S, T, R, SIGMA, Q, *model, N, n, seed, path_major=layout == "path_major")
            raw = np.ascontiguousarray(m).astype("<f8").tobytes()
            assert list(m.shape) == want["shape"], (label, layout)
            if "first_row" in want:
                assert hex_words(m[0]) == want["first_row"] and hex_words(m[-1]) == want["last_row"], (label, layout)
            assert hashlib.sha256(raw).hexdigest() == want["sha256"], (label, layout)      # every word of the matrix


# --------------------------------------------------------------------------------- 9. refusals and NaN at the C ABI ----
def test_refusals_at_the_c_abi():
    """Every refusal of include/olmc_jump.h by its message (the list lives in tests/test_jump_payoffs_cpu.py, which runs it without a
    device), here on an initialised library: nothing is launched, and the next call gives what it gives on its own."""
    from tests.test_jump_payoffs_cpu import test_every_refusal_answers_its_message_before_any_device_work as every_refusal

    N, n, seed = 100, 12, 1
    before = european(M0, "call", N, n, seed)
    every_refusal(_hip.lib())
    after = european(M0, "call", N, n, seed)
    assert (after.n, after.sum, after.sumsq) == (before.n, before.sum, before.sumsq)
    assert after.sum == pytest.approx(_hip.jump_diffusion(S, K, T, R, SIGMA, Q, True, *M0, N, n, seed).sum, **TIE)


def test_nan_inputs_answer_nan():
    N, n, seed = 1000, 13, 2
    nan = float("nan")
    up_out = _hip.BARRIER_KINDS["up-and-out"]
    asian = _hip.PATH_ASIAN_ARITHMETIC
    for model in (M0, K0):
        assert math.isnan(_hip.jd_price(nan, K, T, R, SIGMA, Q, True, model, asian, 0.0, N, n, seed).price)
        assert math.isnan(_hip.jd_price(S, K, T, R, nan, Q, True, model, EUROPEAN, 0.0, N, n, seed, True).price)
        assert math.isnan(_hip.jd_price(S, K, T, R, SIGMA, Q, True, (model[0], nan) + model[2:], asian, 0.0, N, n, seed).price)
        assert math.isnan(_hip.jd_price(S, K, T, R, SIGMA, Q, True, model, up_out, nan, N, n, seed).price)
        for payoff in (_hip.LOOKBACK_FIXED, _hip.LOOKBACK_FLOATING, asian, _hip.PATH_ASIAN_GEOMETRIC):       # ignored there
            st = _hip.jd_price(S, K, T, R, SIGMA, Q, True, model, payoff, nan, N, n, seed)
            assert math.isfinite(st.price) and st.sum == _hip.jd_price(S, K, T, R, SIGMA, Q, True, model, payoff, 0.0, N, n, seed).sum
        for bad in ((nan, T, R, SIGMA, Q), (S, T, R, nan, Q)):
            assert all(math.isnan(st.price) for st in _hip.jd_surface_prices(*bad, True, model, [K, 95.0], [n, 4], N, n, seed))
            assert math.isnan(_hip.jd_autocallable(*bad, model, *AUTOCALL, 4, N, n, seed).price)
            assert math.isnan(_hip.jd_cliquet(*bad, model, *CLIQUET, 4, N, n, seed, True).price)
        nan_model = (model[0], nan) + model[2:]
        assert all(math.isnan(st.price) for st in _hip.jd_surface_prices(S, T, R, SIGMA, Q, True, nan_model, [K], [n], N, n, seed))
        assert math.isnan(_hip.jd_autocallable(S, T, R, SIGMA, Q, nan_model, *AUTOCALL, 4, N, n, seed).price)
        assert math.isnan(_hip.jd_cliquet(S, T, R, SIGMA, Q, nan_model, *CLIQUET, 4, N, n, seed).price)
