"""HestonPricer on scrambled-Sobol paths (method="qmc"), tied per path to a NumPy oracle.

The oracle is written out here: SciPy's Sobol(d=2n, scramble=True, seed).random(N), the clip and norm.ppf of
src/simulation/gbm_qmc.py:32-38, the dimension assignment pinned in include/olmc.h ("quasi-Monte Carlo Heston": sequential =
dimensions 2t, 2t + 1 are Z1, Z2' of step t; bridge = W1 on the even and W2 on the odd dimensions of the breadth-first plan, step t
taking their increments), then the LITERAL recursion of src/pricing_models/heston.py:230-244.  The mirror is the same on -z.

Every path and date counts: the payoff and the full truncation are continuous, there are no near-ties to leave out.  Bars: spot 1e-10
relative, variance 1e-10 absolute, the payoff sum 1e-10 relative (the project's QMC bar); on the CPU the literal and the folded forms
of the recursion differ by at most 1.1e-13 in ln S and 5e-14 in v over these models and n up to 1024.
"""
import collections
import math

import numpy as np
import pytest

from optionslab_amd import _hip
from optionslab_amd.monte_carlo import sobol_tables
from tests.gpu_support import heston_pricer as pricer
from tests.sobol_reference import bridge_walk, normal_chunks

pytestmark = pytest.mark.gpu

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
# kappa theta sigma_v rho v0
USUAL = (2.0, 0.04, 0.3, -0.7, 0.04)
MODELS = [USUAL, (3.0, 0.02, 0.8, 0.3, 0.05), (1.0, 0.04, 1.0, -0.9, 0.04)]         # the second violates Feller's condition
SEEDS = (7, 1234, 2**31 - 5)
COUNTS = (1, 1000, 1 << 14)
STEPS = (1, 2, 13, 64, 252, 1000, 1024, 4096)                                      # 4096: sequential only (the bridge's cap is 1024)


def constructions(n):
    return ("bridge", "sequential") if n <= 1024 else ("sequential",)


# ----------------------------------------------------------------------------------------------------------- oracle ----
def step_normals(z, construction):
    """(Z1, Z2') of every step, each (m, n), from the point's 2n normals."""
    if construction == "sequential":
        return z[:, 0::2], z[:, 1::2]
    return np.diff(bridge_walk(z[:, 0::2]), axis=1), np.diff(bridge_walk(z[:, 1::2]), axis=1)


def literal_recursion(z1, z2p, model, n, S_=S, T_=T, r=R, q=Q):
    """heston.py:291-303 with the given normals: spot and variance, each (m, n + 1)."""
    kappa, theta, sigma_v, rho, v0 = model
    dt = T_ / n
    sqrt_dt = np.sqrt(dt)
    rho_sqrt = np.sqrt(1 - rho**2)
    m = z1.shape[0]
    spot, var = np.zeros((m, n + 1)), np.zeros((m, n + 1))
    spot[:, 0], var[:, 0] = S_, v0
    log_S = np.log(S_) * np.ones(m)
    v = v0 * np.ones(m)
    for t in range(1, n + 1):
        Z1 = z1[:, t - 1]
        Z2 = rho * Z1 + rho_sqrt * z2p[:, t - 1]
        v_pos = np.maximum(v, 0)
        sqrt_v = np.sqrt(v_pos)
        log_S += (r - q - 0.5 * v_pos) * dt + sqrt_v * sqrt_dt * Z1
        v += kappa * (theta - v_pos) * dt + sigma_v * sqrt_v * sqrt_dt * Z2
        v = np.maximum(v, 0)
        spot[:, t] = np.exp(log_S)
        var[:, t] = v
    return spot, var


def oracle_paths(n, n_points, seed, model, chunk=2048, z=None):
    """{(construction, leg): (spot, var)} over Sobol points [0, n_points); leg 1 is the mirror -z.  With z (n_points, 2n) given, over
    the points whose normals are its rows."""
    parts = collections.defaultdict(list)
    for z in normal_chunks(2 * n, n_points, seed, chunk, z):
        for construction in constructions(n):
            z1, z2p = step_normals(z, construction)
            for leg, sign in enumerate((1.0, -1.0)):
                parts[(construction, leg)].append(literal_recursion(sign * z1, sign * z2p, model, n))
    return {key: (np.concatenate([p[0] for p in v]), np.concatenate([p[1] for p in v])) for key, v in parts.items()}


def payoffs(spot, is_call):
    return np.maximum(spot[:, -1] - K, 0) if is_call else np.maximum(K - spot[:, -1], 0)


def device_stats(model, n, n_points, seed, construction, is_call=True, antithetic=False, point_offset=0):
    sv, shift = sobol_tables(2 * n, seed, point_offset + n_points)
    return _hip.heston_qmc(S, K, T, R, Q, is_call, *model, n_points, sv, shift, construction == "bridge", antithetic, point_offset)


def check_paths(got, want, label):
    (spot, var), (spot_o, var_o) = got, want
    assert spot.shape == spot_o.shape and var.shape == var_o.shape
    rel = float(np.max(np.abs(spot - spot_o) / spot_o))
    dv = float(np.max(np.abs(var - var_o)))
    print(label, "max spot rel", rel, "max var abs", dv)
    assert rel <= 1e-10 and dv <= 1e-10, (label, rel, dv)


# ------------------------------------------------------------------------------------- 1. per-path tie to the oracle ----
@pytest.mark.parametrize("n", STEPS)
def test_paths_and_payoff_sums_match_the_oracle(n):
    """Every n meets every model, every N and every seed once; both constructions, both legs, call and put, both layouts."""
    ni = STEPS.index(n)
    for mi, model in enumerate(MODELS):
        N, seed = COUNTS[(ni + mi) % 3], SEEDS[(ni + 2 * mi) % 3]
        oracle = oracle_paths(n, N, seed, model)
        p = pricer(model)
        for construction in constructions(n):
            label = (n, N, seed, model, construction)
            got = p.simulate_paths(S, T, R, Q, N, n, seed, method="qmc", path_construction=construction)
            check_paths(got, oracle[(construction, 0)], label)
            sv, shift = sobol_tables(2 * n, seed, N)                                 # the time-major layout: the same bits, transposed
            spot_t, var_t = _hip.heston_qmc_paths(S, T, R, Q, *model, N, sv, shift, construction == "bridge", path_major=False)
            assert spot_t.shape == (n + 1, N) and np.array_equal(spot_t.T, got[0]) and np.array_equal(var_t.T, got[1])
            del spot_t, var_t
            for is_call in (True, False):
                x0, x1 = payoffs(oracle[(construction, 0)][0], is_call), payoffs(oracle[(construction, 1)][0], is_call)
                for antithetic, x in ((False, x0), (True, np.concatenate([x0, x1]))):
                    st = device_stats(model, n, N, seed, construction, is_call, antithetic)
                    want = float(np.sum(x))
                    print(label, "call" if is_call else "put", "antithetic" if antithetic else "plain", "sum", st.sum, "oracle", want)
                    assert st.n == len(x)
                    assert st.sum == pytest.approx(want, rel=1e-10, abs=1e-12), (label, is_call, antithetic)
                    assert st.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10, abs=1e-12)
                    price = p.price_monte_carlo(S, K, T, R, Q, "call" if is_call else "put", N, n, seed, antithetic, method="qmc",
                                                path_construction=construction)
                    assert isinstance(price, np.float64)
                    assert float(price) == pytest.approx(math.exp(-R * T) * float(np.mean(x)), rel=1e-10, abs=1e-12)


def test_a_negative_start_variance_keeps_the_reference_recursion_at_the_c_abi():
    """HestonPricer refuses v0 < 0; the C ABI keeps heston.py's arithmetic: the first step sees v+ = 0 and is deterministic."""
    model = (2.0, 0.04, 0.3, -0.7, -0.01)
    for n, N, seed in ((13, 1000, 7), (252, 1000, 1234)):
        oracle = oracle_paths(n, N, seed, model)
        sv, shift = sobol_tables(2 * n, seed, N)
        for construction in constructions(n):
            got = _hip.heston_qmc_paths(S, T, R, Q, *model, N, sv, shift, construction == "bridge", path_major=True)
            check_paths(got, oracle[(construction, 0)], (n, "v0 < 0", construction))
            assert np.all(got[1][:, 0] == -0.01) and np.all(got[1][:, 1] == got[1][0, 1])      # date 1 is the same on every path
            x = np.concatenate([payoffs(oracle[(construction, leg)][0], True) for leg in (0, 1)])
            st = device_stats(model, n, N, seed, construction, True, True)
            assert st.sum == pytest.approx(float(np.sum(x)), rel=1e-10, abs=1e-12)


def test_return_error_is_the_naive_standard_error():
    n, N, seed = 64, 1000, 7
    x = payoffs(oracle_paths(n, N, seed, USUAL)[("bridge", 0)][0], True)
    price, err = pricer(USUAL).price_monte_carlo(S, K, T, R, Q, "call", N, n, seed, return_error=True, method="qmc")
    assert float(price) == pytest.approx(math.exp(-R * T) * float(np.mean(x)), rel=1e-10)
    assert err == pytest.approx(math.exp(-R * T) * float(np.std(x)) / math.sqrt(N), rel=1e-6)


# -------------------------------------------------------------------------------------------------- 2. consistency ----
@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_the_price_is_the_discounted_mean_payoff_of_the_paths_last_column(construction):
    # the two kernels add the drift n (r - q) dt to ln S in a different order: a few ulps of ln S per path, far inside the QMC bar
    p = pricer(USUAL)
    for n, N, seed in ((252, 1 << 14, 11), (50, 1000, 12), (1024, 4097, 13)):
        spot, _var = p.simulate_paths(S, T, R, Q, N, n, seed, method="qmc", path_construction=construction)
        for option_type in ("call", "put"):
            x = payoffs(spot, option_type == "call")
            got = p.price_monte_carlo(S, K, T, R, Q, option_type, N, n, seed, method="qmc", path_construction=construction)
            assert float(got) == pytest.approx(math.exp(-R * T) * float(np.mean(x)), rel=1e-10)


def test_equal_seeds_give_equal_bits():
    p = pricer(USUAL)
    for construction in ("bridge", "sequential"):
        for antithetic in (False, True):
            price = lambda seed, n=252: p.price_monte_carlo(S, K, T, R, Q, "call", 1 << 14, n, seed, antithetic, method="qmc",
                                                            path_construction=construction)
            first = price(11)
            other = price(12)
            price(12, 100)                                                          # other tables, another plan, other slabs in between
            assert price(11) == first and price(12) == other and first != other
        a = p.simulate_paths(S, T, R, Q, 1000, 64, 5, method="qmc", path_construction=construction)
        b = p.simulate_paths(S, T, R, Q, 1000, 64, 5, method="qmc", path_construction=construction)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_shards_of_one_sequence_add_up(construction):
    n, N, a = 252, 1 << 14, 4321                        # a: neither a multiple of 64 nor of 512
    for model, is_call, antithetic in ((USUAL, True, False), (USUAL, False, True), (MODELS[1], True, True), (MODELS[2], False, False)):
        call = lambda off, cnt: device_stats(model, n, cnt, 5, construction, is_call, antithetic, point_offset=off)
        whole, lo, hi = call(0, N), call(0, a), call(a, N - a)
        assert whole.n == lo.n + hi.n
        assert whole.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12)
        assert whole.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12)


def test_pseudo_is_bit_for_bit_what_it_was():
    N, n, seed = 1 << 14, 252, 77
    p = pricer(USUAL)
    want = _hip.heston(S, K, T, R, Q, True, *USUAL, N, n, seed, False)
    want_a = _hip.heston(S, K, T, R, Q, False, *USUAL, N, n, seed, True)
    spot, var = _hip.heston_paths(S, T, R, Q, *USUAL, 1000, n, seed, path_major=True)
    for kw in (dict(), dict(method="pseudo"), dict(method="pseudo", path_construction="sequential")):
        assert float(p.price_monte_carlo(S, K, T, R, Q, "call", N, n, seed, **kw)) == want.price
        got = p.price_monte_carlo(S, K, T, R, Q, "put", N, n, seed, True, True, **kw)
        assert (float(got[0]), got[1]) == (want_a.price, want_a.std_error)
        s2, v2 = p.simulate_paths(S, T, R, Q, 1000, n, seed, **kw)
        assert np.array_equal(s2, spot) and np.array_equal(v2, var)


def test_with_profiling_on_every_heston_launch_counts_once_in_the_kernel_time():
    """The launch timer tools/heston_qmc_timing.py reads: one timed launch per call, the path matrices' too, Philox and Sobol."""
    N, n = 1000, 64
    sv, shift = sobol_tables(2 * n, 1, N)
    calls = [lambda: _hip.heston(S, K, T, R, Q, True, *USUAL, N, n, 1, False), lambda: _hip.heston_paths(S, T, R, Q, *USUAL, N, n, 1)]
    for bridge in (True, False):
        calls.append(lambda b=bridge: _hip.heston_qmc(S, K, T, R, Q, True, *USUAL, N, sv, shift, b, True))
        calls.append(lambda b=bridge: _hip.heston_qmc_paths(S, T, R, Q, *USUAL, N, sv, shift, b))
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
    _hip.heston_paths(S, T, R, Q, *USUAL, N, n, 1)
    assert _hip.kernel_time()[0] == 0                                               # profiling off: nothing is timed


# --------------------------------------------------------------------------------------------- 3. the point of the feature ----
@pytest.mark.parametrize("N,n", [(1 << 14, 252), (1 << 12, 64)])
def test_the_bridge_beats_pseudo_random_paths_and_agrees_with_them(N, n):
    """The usual model's ATM call, 16 scrambles against 16 Philox seeds at equal N: the CPU prototype measured a ratio of standard
    deviations of 16.8 (2^14 x 252) and 20 (2^12 x 64); a ratio of two 16-sample standard deviations is off by under 2.3x at the 99.9 %
    level (F distribution), so a true 17x cannot read below 7x.  The bar is 3x.  And the two methods price the same thing: the mean of
    the 16 bridge prices lies within 3 combined standard errors of a Philox price at 2^22 paths."""
    p = pricer(USUAL)
    pseudo = [float(p.price_monte_carlo(S, K, T, R, Q, "call", N, n, 1000 + s)) for s in range(16)]
    bridge = [float(p.price_monte_carlo(S, K, T, R, Q, "call", N, n, s, method="qmc")) for s in range(16)]
    sd_pseudo, sd_bridge = float(np.std(pseudo, ddof=1)), float(np.std(bridge, ddof=1))
    print(N, n, "pseudo", sd_pseudo, "bridge", sd_bridge, "ratio", sd_pseudo / sd_bridge)
    big, big_err = p.price_monte_carlo(S, K, T, R, Q, "call", 1 << 22, n, 4242, return_error=True)
    mean = float(np.mean(bridge))
    combined = math.hypot(sd_bridge / 4.0, big_err)                                   # the mean of 16 and the Philox price
    print(N, n, "bridge mean", mean, "philox 2^22", float(big), "combined se", combined, "distance", abs(mean - float(big)) / combined)
    assert sd_bridge <= sd_pseudo / 3.0, (sd_bridge, sd_pseudo)
    assert abs(mean - float(big)) <= 3.0 * combined, (mean, float(big), combined)
