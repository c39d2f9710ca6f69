"""Jump-diffusion scenario sets and the fused finite-difference Greeks (include/olmc_jump_scenarios.h, price_scenarios, JumpMCAdapter) on
the device.

Scenario i of a launch is the European contract olmc_jump_diffusion prices with its parameters, the same n_steps and the same seed (with
antithetic: oljd_price's European).  The bars are the project's own (tests/test_gpu_jump_payoffs.py, tests/test_gpu_heston_scenarios.py):
TIE for per-path ties of sums against NumPy -- licensed for the FOLDED sum by tests/test_jump_scenarios_cpu.py, which holds the folded
oracle to the interleaved one at this bar on these very sets and shapes --, rel 1e-12 for sums that must agree with a neighbouring kernel or
add up, == where bits must not change.  The sets, the models and the scaling of the maturities at n = 1, 2 (the Kou model has 60 jumps a
year and the library takes at most 20 a step) are tests/jump_scenario_cases.py's.

 1. Every scenario's sums against the NumPy payoffs of the last column of the device's own path matrix for its parameters.
 2. The mirror leg: both legs' matrices.   3. Neighbours: each scenario alone against olmc_jump_diffusion / oljd_price.
 4. Independence of the scenarios, of their order, of the group bound and of the cut.   5. Shards.
 6. Grid stride: the uncapped words under a cap of one up to eight trips, the uncapped sums to their reassociation elsewhere.
 7. Fused = literal Greeks.   8. One launch.   9. NaN.   10. lambda = 0.   11. Merton's series as the analytic anchor.
"""
import math

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.greeks import compute_greeks_unified, fd_steps
from tests import jump_scenario_cases as jc
from tests import jump_scenario_oracle as jo

pytestmark = pytest.mark.gpu

TIE = dict(rel=1e-10, abs=1e-12)
S, K, T, R, Q, SIGMA = jc.S, jc.K, jc.T, jc.R, jc.Q, jc.SIGMA
MERTON, KOU = jc.MERTON, jc.KOU
GREEK_NAMES = ("price", "delta", "gamma", "vega", "theta", "rho", "vanna", "charm", "vomma")
scenario = jc.scenario


def public_model(model):
    return ol.KouJumpDiffusion(*model[1:]) if model[0] else ol.MertonJumpDiffusion(*model[1:4])


def words(st):
    return (st.sum, st.sumsq, st.n, st.price, st.std_error)


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


def last_column(sc, N, n, seed, cache, mirror=False):
    """The last column of the device's own path matrix of the scenario's (S, T, r, sigma, q, model)."""
    key = (sc[0], *sc[2:6], *sc[7:], mirror)
    if key not in cache:
        if mirror:
            spot = _hip.jd_paths(sc[0], sc[2], sc[3], sc[4], sc[5], sc[7:], N, n, seed, mirror=True, path_major=True)
        else:
            spot = _hip.jump_paths(sc[0], sc[2], sc[3], sc[4], sc[5], *sc[7:], N, n, seed, path_major=True)
        cache[key] = spot[:, n].copy()
    return cache[key]


def test_the_sets_are_what_the_tests_below_take_them_for():
    for model in jc.MODELS.values():
        assert _hip.jd_scenario_layout(jc.greeks_set(model)) == (2, [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1])
        assert _hip.jd_scenario_layout(jc.mixed_set(model)) == jc.mixed_groups() and jc.mixed_groups()[0] == 7
    for n in jc.TIE_STEPS:
        for scenarios in jc.tie_sets(n).values():
            assert all(sc[8] * sc[2] / n <= 20.0 for sc in scenarios)


# -------------------------------------------------------------------------------------- 1. tie to the device's own matrix ----
@pytest.mark.parametrize("n", jc.TIE_STEPS)
def test_scenarios_match_the_last_column_of_the_devices_own_path_matrices(n):
    for N in jc.TIE_PATHS:
        seed = jc.tie_seed(n, N)
        cache = {}
        for name, scenarios in jc.tie_sets(n).items():
            stats = _hip.jd_scenarios(scenarios, N, n, seed)
            assert len(stats) == len(scenarios)
            for i, (st, sc) in enumerate(zip(stats, scenarios)):
                check_stats(st, jo.payoff(last_column(sc, N, n, seed, cache), sc), sc, (name, n, N, i))


# ------------------------------------------------------------------------------------------------------ 2. the mirror leg ----
@pytest.mark.parametrize("N,n", jc.MIRROR_SHAPES)
def test_with_antithetic_the_sums_are_those_of_both_legs_matrices(N, n):
    seed = 7 * n + N
    cache = {}
    for name, scenarios in jc.tie_sets(n).items():
        stats = _hip.jd_scenarios(scenarios, N, n, seed, True)
        for i, (st, sc) in enumerate(zip(stats, scenarios)):
            x = np.concatenate([jo.payoff(last_column(sc, N, n, seed, cache, mirror), sc) for mirror in (False, True)])
            check_stats(st, x, sc, (name, n, N, i))


# ---------------------------------------------------------------------------------------------------------- 3. neighbours ----
def test_a_scenario_alone_is_the_one_contract_kernels_price():
    N, n, seed = 4097, 64, 5
    for model in jc.MODELS.values():
        for sc in jc.greeks_set(model) + jc.mixed_set(model):
            for antithetic in (False, True):
                got = _hip.jd_scenarios([sc], N, n, seed, antithetic)[0]
                if antithetic:
                    one = _hip.jd_price(*sc[:7], sc[7:], _hip.JD_EUROPEAN, 0.0, N, n, seed, True)
                else:
                    one = _hip.jump_diffusion(*sc[:7], *sc[7:], N, n, seed)
                assert got.n == one.n
                assert got.sum == pytest.approx(one.sum, rel=1e-12) and got.sumsq == pytest.approx(one.sumsq, rel=1e-12), sc
                assert got.price == pytest.approx(one.price, rel=1e-12) and got.std_error == pytest.approx(one.std_error, rel=1e-9), sc


def test_price_scenarios_is_price_monte_carlo_scenario_by_scenario():
    N, n, seed = 4097, 64, 21
    for model in jc.MODELS.values():
        p = public_model(model)
        scenarios = [jc.as_mapping(sc) for sc in jc.mixed_set(model) if sc[7] == model[0]]
        scenarios.append(dict(S=S, K=K, T=T, r=R, sigma=SIGMA))                        # the instance's own model, q = 0, a call
        for antithetic in (False, True):
            prices, errors = p.price_scenarios(scenarios, N, n, seed, antithetic, return_error=True)
            assert prices.shape == errors.shape == (len(scenarios),) and prices.dtype == np.float64
            assert np.array_equal(prices, p.price_scenarios(scenarios, N, n, seed, antithetic))
            for i, sc in enumerate(scenarios):
                fields = {key: sc[key] for key in ("lambda_j", "mu_j", "sigma_j", "p", "eta1", "eta2") if key in sc}
                one = type(p)(**{**{f: getattr(p, f) for f in p.__dataclass_fields__}, **fields})
                want, want_error = one.price_monte_carlo(sc["S"], sc["K"], sc["T"], sc["r"], sc["sigma"], sc.get("option_type", "call"), sc.get("q", 0.0),
                                                         N, n, seed, True, antithetic=antithetic)
                assert prices[i] == pytest.approx(float(want), rel=1e-12) and errors[i] == pytest.approx(want_error, rel=1e-9), sc


# -------------------------------------------------------------------------------------------------------- 4. independence ----
def test_a_scenario_does_not_depend_on_its_neighbours_its_place_the_group_bound_or_the_cut():
    N, n, seed = 4097, 64, 31
    for model in jc.MODELS.values():
        scenarios = jc.mixed_set(model)                                              # seven groups: the bound of sixteen
        _n_groups, group = jc.mixed_groups()
        bits = [words(st) for st in _hip.jd_scenarios(scenarios, N, n, seed, True)]
        for i, sc in enumerate(scenarios):                                           # alone: one group, the bound of two, slot 0
            assert words(_hip.jd_scenarios([sc], N, n, seed, True)[0]) == bits[i], i
        for st, want in zip(_hip.jd_scenarios(scenarios[::-1], N, n, seed, True), bits[::-1]):      # other slots, other group numbers
            assert words(st) == want
        pair = _hip.jd_scenarios([scenarios[4], scenarios[1]], N, n, seed, True)     # two groups: the bound of two
        assert [words(st) for st in pair] == [bits[4], bits[1]]
        four = [i for i in range(16) if group[i] in (0, 2, 4, 5)]                    # four groups: the bound of four
        assert _hip.jd_scenario_layout([scenarios[i] for i in four])[0] == 4
        assert [words(st) for st in _hip.jd_scenarios([scenarios[i] for i in four], N, n, seed, True)] == [bits[i] for i in four]
        three = [i for i in range(16) if group[i] in (1, 3, 6)]                      # three groups in the bound of four
        assert [words(st) for st in _hip.jd_scenarios([scenarios[i] for i in three], N, n, seed, True)] == [bits[i] for i in three]
        # sixteen groups in one launch: every scenario of the mixed set at a maturity of its own
        spread = [(*sc[:2], sc[2] * (1.0 + i / 64.0), *sc[3:]) for i, sc in enumerate(scenarios)]
        assert _hip.jd_scenario_layout(spread)[0] == 16
        for sc, st in zip(spread, _hip.jd_scenarios(spread, N, n, seed, True)):
            assert words(st) == words(_hip.jd_scenarios([sc], N, n, seed, True)[0])
    # the cut of a 40-scenario list into launches of 16, 16 and 8
    p = public_model(MERTON)
    forty = [jc.as_mapping(sc) for sc in jc.mixed_set(MERTON) if not sc[7]] * 4
    forty = [dict(sc, K=sc["K"] + 0.25 * i) for i, sc in enumerate(forty)][:40]
    assert len(forty) == 40
    prices, errors = p.price_scenarios(forty, N, n, seed, True, return_error=True)
    for i in (0, 15, 16, 17, 31, 32, 39):
        alone = p.price_scenarios([forty[i]], N, n, seed, True, return_error=True)
        assert (prices[i], errors[i]) == (alone[0][0], alone[1][0]), i
    shifted = p.price_scenarios(forty[3:], N, n, seed, True)
    assert np.array_equal(shifted, prices[3:])


# --------------------------------------------------------------------------------------------------------------- 5. shards ----
def test_uneven_shards_add_up_and_equal_arguments_give_equal_words():
    N, n, a, seed = 4097, 64, 1000, 9                                                # a is no multiple of 64
    for model, antithetic, base in ((MERTON, False, 0), (KOU, True, (1 << 32) + 12345)):
        scenarios = jc.mixed_set(model)
        call = lambda off, cnt: _hip.jd_scenarios(scenarios, cnt, n, seed, antithetic, base + off)
        whole = call(0, N)
        assert [words(st) for st in call(0, N)] == [words(st) for st in whole]
        for full, lo, hi, sc in zip(whole, call(0, a), call(a, N - a), scenarios):
            assert full.n == lo.n + hi.n == N * (2 if antithetic else 1)
            assert full.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12), sc
            assert full.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12), sc
            combined = _hip.combine_stats([(lo.sum, lo.sumsq, lo.n), (hi.sum, hi.sumsq, hi.n)], sc[3], sc[2])     # the scenario's own r, T
            assert combined.price == pytest.approx(full.price, rel=1e-12)
        if base:                                                                     # beyond 2^32 the paths are others, and the single contract's
            assert [st.sum for st in whole] != [st.sum for st in _hip.jd_scenarios(scenarios, N, n, seed, antithetic, 12345)]
            one = _hip.jd_price(*scenarios[0][:7], scenarios[0][7:], _hip.JD_EUROPEAN, 0.0, N, n, seed, True, base)
            assert whole[0].sum == pytest.approx(one.sum, rel=1e-12)
    run = lambda s, n_=64, N_=4097: [words(st) for st in _hip.jd_scenarios(jc.mixed_set(KOU), N_, n_, s, True)]
    first, other = run(11), run(12)
    run(12, 100, 1000)                                                               # another grid in between
    assert run(11) == first and run(12) == other and first != other


# ---------------------------------------------------------------------------------------------------------- 6. grid stride ----
def launches(sets, N, n, seed):
    return [[words(st) for st in _hip.jd_scenarios(sc, N, n, seed, anti)] for sc in sets for anti in (False, True)]


def capped_launches(cap, sets, N, n, seed):
    _hip.tune(_hip.TUNE_GRID_CAP, cap)
    try:
        return launches(sets, N, n, seed)
    finally:
        _hip.tune(_hip.TUNE_GRID_CAP, 0)                                             # the knob is process-global: 0 again whatever happens


def test_under_a_grid_cap_of_one_the_trips_give_the_uncapped_words():
    """1200 paths: five trips of the one workgroup, the last with two whole waves, a ragged one and an idle one.  A workgroup adds its
    trips' rows in trip order and the grid reduction adds up to eight workgroups' rows in index order: the same sum, word for word."""
    N, n, seed = 1200, 13, 17
    sets = [jc.greeks_set(KOU), jc.mixed_set(MERTON), jc.mixed_set(KOU)]
    assert capped_launches(1, sets, N, n, seed) == launches(sets, N, n, seed)


def test_under_other_caps_and_sizes_the_trips_give_the_uncapped_sums_to_their_reassociation():
    """tests/test_gpu_grid_stride.py's bar: two rounded fp64 sums of the same n non-negative terms differ by at most 2 gamma / (1 - gamma)
    of either, gamma = n u / (1 - n u), u = 2^-53.  4133 paths: 17 trips under a cap of 1, six (the last ragged) under a cap of 3."""
    N, n, seed = 4133, 13, 17
    sets = [jc.greeks_set(KOU), jc.mixed_set(MERTON), jc.mixed_set(KOU)]
    free = launches(sets, N, n, seed)
    for cap in (1, 3):
        for got, want in zip(capped_launches(cap, sets, N, n, seed), free):
            for g, w in zip(got, want):
                gamma = w[2] * 2.0**-53 / (1.0 - w[2] * 2.0**-53)
                tol = 2.0 * gamma / (1.0 - gamma)
                assert g[2] == w[2] and abs(g[0] - w[0]) <= tol * w[0] and abs(g[1] - w[1]) <= tol * w[1], (cap, g, w)
                assert g[3] == pytest.approx(w[3], rel=1e-12)


# ------------------------------------------------------------------------------------------------------- 7. fused = literal ----
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


class Recording(ol.JumpMCAdapter):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def price(self, S_, K_, T_, r_, sigma, option_type, q=0.0, **kw):
        value = super().price(S_, K_, T_, r_, sigma, option_type, q, **kw)
        self.calls.append(((S_, T_, r_, sigma), float(value)))
        return value


@pytest.mark.parametrize("antithetic", (False, True), ids=["plain", "antithetic"])
@pytest.mark.parametrize("model", list(jc.MODELS))
@pytest.mark.parametrize("T_,second", [(1.0, True), (1.0, False), (1 / 400, True)], ids=["second-order", "first-order", "short"])
def test_the_fused_greeks_are_the_literal_ones(T_, second, model, antithetic):
    N, n, seed, sigma = 4097, 64, 41, 0.25
    m = jc.MODELS[model]
    p = public_model(m)
    option_type = "call" if model == "merton" else "put"
    out9, evals = _hip.jd_greeks_fd(S, K, T_, R, sigma, Q, option_type == "call", m, N, n, seed, antithetic, second, want_evals=True)
    bumps = jc.greeks_bumps(sigma, T_, second)
    assert len(evals) == 14 and len(bumps) == {(1.0, True): 14, (1.0, False): 8, (1 / 400, True): 11}[(T_, second)]
    for st in evals[len(bumps):]:
        assert words(st) == (0.0, 0.0, 0, 0.0, 0.0)
    # the literal price_monte_carlo calls with the same seed
    for st, (s, t, r, v) in zip(evals, bumps):
        want, want_error = p.price_monte_carlo(s, K, t, r, v, option_type, Q, N, n, seed, True, antithetic=antithetic)
        assert st.n == N * (2 if antithetic else 1)
        assert st.price == pytest.approx(float(want), rel=1e-12) and st.std_error == pytest.approx(want_error, rel=1e-9), (s, t, r, v)
    want9 = finite_differences([st.price for st in evals], T_, second)
    assert list(out9[:len(want9)]) == want9
    # the adapter: one launch, the same nine numbers; fused=False the call-by-call way
    adapter = Recording(p, N, n, seed, antithetic)
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
    if T_ == 1.0 and second:
        wrapped = ol.greeks_jump_monte_carlo(p, S, K, T_, R, sigma, option_type, Q, n_paths=N, n_steps=n, seed=seed, antithetic=antithetic)
        assert [float(v) for v in wrapped.values()] == want9


# ---------------------------------------------------------------------------------------------------------- 8. one launch ----
def test_with_profiling_on_every_entry_point_counts_once_in_the_kernel_time():
    N, n, seed = 1000, 64, 1
    scenarios = jc.mixed_set(KOU)
    calls = [lambda: _hip.jd_scenarios(scenarios, N, n, seed, True), lambda: _hip.jd_scenarios(scenarios[:1], N, n, seed),
             lambda: _hip.jd_greeks_fd(S, K, T, R, SIGMA, Q, True, KOU, N, n, seed, True, True),
             lambda: _hip.jd_greeks_fd(S, K, T, R, SIGMA, Q, False, MERTON, N, n, seed, False, False, want_evals=False)]
    _hip.profile_enable(True)
    try:
        for call in calls:
            _hip.profile_reset()
            call()
            launches, ms = _hip.kernel_time()
            assert launches == 1 and ms > 0.0
        _hip.profile_reset()
        _hip.jd_scenario_layout(scenarios)                                           # host arithmetic: no launch
        assert _hip.kernel_time()[0] == 0
    finally:
        _hip.profile_enable(False)
    _hip.profile_reset()


# ----------------------------------------------------------------------------------------------------------------- 9. NaN ----
def test_a_nan_poisons_its_own_scenario_only():
    N, n, seed = 1000, 13, 3
    nan = float("nan")
    for model in jc.MODELS.values():
        base = [scenario(model=model), scenario(101.0, 95.0, 0.5, 0.03, 0.25, 0.01, False, model), scenario(K_=110.0, model=model),
                scenario(99.0, 105.0, 1.0, R, 0.3, Q, False, KOU if model is MERTON else MERTON), scenario(101.0, 90.0, 0.5, 0.03, 0.25, 0.01, True, model)]
        for antithetic in (False, True):
            first = _hip.jd_scenarios(base, N, n, seed, antithetic)
            clean = [words(st) for st in first]
            assert all(math.isfinite(v) for row in clean for v in row)
            for field in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):                           # S K T r sigma q, then lambda_j a1 a2 a3
                poisoned = list(base)
                poisoned[1] = (*base[1][:field], nan, *base[1][field + 1:])
                got = _hip.jd_scenarios(poisoned, N, n, seed, antithetic)
                assert math.isnan(got[1].price) and math.isnan(got[1].std_error) and math.isnan(got[1].sum) and got[1].n == first[1].n, field
                assert [words(st) for i, st in enumerate(got) if i != 1] == clean[:1] + clean[2:], field
    # a negative spot answers NaN as everywhere else (poisoned())
    got = _hip.jd_scenarios([scenario(), scenario(S_=-1.0)], N, n, seed)
    assert math.isnan(got[1].price) and got[0].price == _hip.jd_scenarios([scenario()], N, n, seed)[0].price


# ---------------------------------------------------------------------------------------------------------- 10. lambda = 0 ----
@pytest.mark.parametrize("antithetic", (False, True))
def test_a_group_without_jumps_next_to_a_jumping_one_is_the_gbm_price(antithetic):
    N, n, seed = 1 << 16, 32, 8                                                      # tests/test_gpu_jump_payoffs.py's anchor shape, and its bar
    for quiet in ((False, 0.0, -0.1, 0.2, 0.0), (True, 0.0, 0.4, 10.0, 5.0)):
        for call in (True, False):
            got = _hip.jd_scenarios([scenario(call=call, model=KOU), scenario(call=call, model=quiet), scenario(call=call, model=MERTON)], N, n, seed, antithetic)
            st = got[1]
            z = (st.price - ol.black_scholes(S, K, T, R, SIGMA, "call" if call else "put", Q)) / st.std_error
            print("quiet", quiet[0], "call", call, "antithetic", antithetic, "z", z)
            assert abs(z) <= 3.5
            one = _hip.jd_price(S, K, T, R, SIGMA, Q, call, quiet, _hip.JD_EUROPEAN, 0.0, N, n, seed, antithetic)
            assert st.price == pytest.approx(one.price, rel=1e-12)
            assert got[0].price != st.price != got[2].price


# ------------------------------------------------------------------------------------------------- 11. the analytic anchor ----
def test_the_greeks_of_the_monte_carlo_price_meet_those_of_mertons_series():
    """For each of the nine Greeks the mean of greeks_jump_monte_carlo over 16 fixed seeds (2^16 paths x 16 steps) within 5 standard
    errors of that mean -- the scatter over the 16 runs / 4 -- of compute_greeks_unified over Merton's series price.  The simulation is
    exact in distribution for a European (compound Poisson per step; the count cap of 64 is out of reach at lambda dt <= 20): no
    discretisation bias enters the bound.  Five: a scatter estimated from 16 runs is itself uncertain by about a fifth."""
    p = public_model(MERTON)
    for option_type, antithetic in (("call", False), ("put", True)):
        want = compute_greeks_unified(ol.JumpDiffusionAdapter(p), S, K, T, R, SIGMA, option_type, Q)
        runs = np.asarray([[float(v) for v in ol.greeks_jump_monte_carlo(p, S, K, T, R, SIGMA, option_type, Q, n_paths=1 << 16, n_steps=16, seed=900 + s,
                                                                         antithetic=antithetic).values()] for s in range(16)])
        assert runs.shape == (16, 9) and list(want) == list(GREEK_NAMES)
        for j, name in enumerate(GREEK_NAMES):
            mean, err = float(np.mean(runs[:, j])), float(np.std(runs[:, j], ddof=1) / 4.0)
            print(option_type, name, "mean", mean, "series", float(want[name]), "distance / (5 err)", abs(mean - float(want[name])) / (5.0 * err))
            assert abs(mean - float(want[name])) <= 5.0 * err, (option_type, name, mean, err, float(want[name]))
