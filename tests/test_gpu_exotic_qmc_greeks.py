"""Fused finite-difference Greeks of the Asian, barrier and lookback payoffs on scrambled-Sobol paths (olmc_asian_qmc_greeks_fd /
olmc_extrema_qmc_greeks_fd, ExoticAdapter(..., method="qmc")): every evaluation of the one launch is the launch of its contract
alone, the adapter's default (fused) path is the literal form's numbers, and the oracle of test_gpu_exotic_qmc anchors both."""
import math
import threading

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.greeks import ExoticAdapter, compute_greeks_unified, fd_steps
from optionslab_amd.monte_carlo import sobol_tables
from tests.test_gpu_exotic_qmc import DOWN, UP, oracle_prices

pytestmark = pytest.mark.gpu

S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0
KINDS = [("asian", "arithmetic"), ("asian", "geometric"), ("barrier", "up-and-out"), ("barrier", "up-and-in"),
         ("barrier", "down-and-out"), ("barrier", "down-and-in"), ("lookback", "floating"), ("lookback", "fixed")]


def bumped_contracts(second_order, S_=S, T_=T, r=R, sigma=SIG):
    """(S, T, r, sigma) of the evaluations in olmc_*_greeks_fd's order (GreeksSet: the reference's get_price() calls)."""
    h_S, h_v, h_r, h_T = fd_steps(S_)
    out = [(S_, T_, r, sigma), (S_ + h_S, T_, r, sigma), (S_ - h_S, T_, r, sigma), (S_, T_, r, sigma + h_v), (S_, T_, r, sigma - h_v)]
    has_T = T_ > h_T
    if has_T:
        out.append((S_, T_ - h_T, r, sigma))
    out += [(S_, T_, r + h_r, sigma), (S_, T_, r - h_r, sigma)]
    if second_order:
        out += [(S_ + h_S, T_, r, sigma + h_v), (S_ + h_S, T_, r, sigma - h_v), (S_ - h_S, T_, r, sigma + h_v), (S_ - h_S, T_, r, sigma - h_v)]
        if has_T:
            out += [(S_ + h_S, T_ - h_T, r, sigma), (S_ - h_S, T_ - h_T, r, sigma)]
    return out


def _payoff(kind, sub):
    if kind == "barrier":
        return _hip.BARRIER_KINDS[sub], (UP if sub.startswith("up") else DOWN)
    return (_hip.LOOKBACK_FLOATING if sub == "floating" else _hip.LOOKBACK_FIXED), 0.0


def fused(kind, sub, is_call, n_points, sv, shift, bridge, anti, second):
    if kind == "asian":
        return _hip.asian_qmc_greeks_fd(S, K, T, R, SIG, Q, is_call, sub == "geometric", n_points, sv, shift, bridge, anti, second)
    payoff, level = _payoff(kind, sub)
    return _hip.extrema_qmc_greeks_fd(S, K, T, R, SIG, Q, is_call, payoff, level, n_points, sv, shift, bridge, anti, second)


def alone(kind, sub, is_call, n_points, sv, shift, bridge, anti, contract):
    S_, T_, r, sigma = contract
    if kind == "asian":
        return _hip.asian_qmc(S_, K, T_, r, sigma, Q, is_call, sub == "geometric", n_points, sv, shift, bridge, anti)
    payoff, level = _payoff(kind, sub)
    return _hip.extrema_qmc(S_, K, T_, r, sigma, Q, is_call, payoff, level, n_points, sv, shift, bridge, anti)


def _check_evaluations(n, construction, n_points, seed, combos):
    sv, shift = sobol_tables(n, seed, n_points)
    bridge = construction == "bridge"
    bad, bitwise = [], {True: 0, False: 0}
    for kind, sub in KINDS:
        for is_call in (True, False):
            for anti, second in combos:
                vals, evals = fused(kind, sub, is_call, n_points, sv, shift, bridge, anti, second)
                contracts = bumped_contracts(second)
                assert all(math.isfinite(v) for v in vals)
                for i, c in enumerate(contracts):
                    want, got = alone(kind, sub, is_call, n_points, sv, shift, bridge, anti, c), evals[i]
                    ok = (got.n == want.n == n_points * (2 if anti else 1) and got.sum == pytest.approx(want.sum, rel=1e-13, abs=1e-300)
                          and got.sumsq == pytest.approx(want.sumsq, rel=1e-13, abs=1e-300))
                    if not ok:
                        bad.append((kind, sub, is_call, anti, second, i, (got.n, got.sum, got.sumsq), (want.n, want.sum, want.sumsq)))
                    if kind != "asian":
                        bitwise[got.sum == want.sum and got.sumsq == want.sumsq] += 1
                for i in range(len(contracts), 14):
                    assert evals[i].n == 0 and evals[i].sum == 0.0
    assert not bad, bad[:8]
    return bitwise


_ALL = [(False, False), (True, False), (False, True), (True, True)]


# --------------------------------------------------------------------------------------- 1. each evaluation is its launch ----
@pytest.mark.parametrize("construction", ["bridge", "sequential"])
@pytest.mark.parametrize("n,n_points", [(1, 1001), (3, 517), (67, 1001), (252, 4099)])
def test_each_evaluation_equals_its_own_launch(construction, n, n_points):
    _check_evaluations(n, construction, n_points, 29 + n, _ALL)


def test_each_evaluation_equals_its_own_launch_beyond_the_bridge_cap():
    _check_evaluations(1500, "sequential", 203, 77, [(True, True), (False, False)])


def test_grid_striding_launches_agree_too():
    # beyond 8192 workgroups x 4 points every wave takes several points
    _check_evaluations(5, "bridge", (1 << 15) + 4097, 5, [(True, True)])


# ---------------------------------------------------------------------------------------------------- 2. the adapter ----
def _option(kind, sub, seed):
    if kind == "asian":
        return ol.AsianOption(S, K, T, R, SIG, Q, seed=seed), {"avg_type": sub}
    if kind == "barrier":
        return ol.BarrierOption(S, K, T, R, SIG, Q, seed=seed, barrier=UP if sub.startswith("up") else DOWN), {"barrier_type": sub}
    return ol.LookbackOption(S, K, T, R, SIG, Q, seed=seed), {"lookback_type": sub}


@pytest.mark.parametrize("kind,sub", KINDS)
@pytest.mark.parametrize("construction,anti,second", [("bridge", False, True), ("sequential", True, False), ("bridge", True, True)])
def test_the_adapter_fuses_by_default_and_matches_the_literal_form(kind, sub, construction, anti, second):
    opt, kw = _option(kind, sub, 4242)
    ad = ExoticAdapter(opt, n_paths=3001, n_steps=48, method="qmc", path_construction=construction, antithetic=anti, **kw)
    assert ad._fused_plan() is not None
    for ot in ("call", "put"):
        got = compute_greeks_unified(ad, S, K, T, R, SIG, ot, Q, include_second_order=second)
        assert (opt.S, opt.K, opt.T, opt.r, opt.sigma, opt.q) == (S, K, T, R, SIG, Q)
        want = compute_greeks_unified(ad, S, K, T, R, SIG, ot, Q, include_second_order=second, fused=False)
        assert list(got) == list(want)
        assert all(type(v) is np.float64 for v in got.values())
        for key in want:
            assert got[key] == pytest.approx(float(want[key]), rel=1e-8, abs=1e-8), (key, ot)
        # the kernel's own values, key by key
        raw, _ = fused(kind, sub, ot == "call", 3001, *sobol_tables(48, 4242, 3001), construction == "bridge", anti, second)
        assert [float(v) for v in got.values()] == raw[:len(got)]


# ------------------------------------------------------------------------------------------ 3. an independent anchor ----
class _OraclePricer:
    def __init__(self, key, n_points, n_steps, seed, bridge):
        self.key, self.n_points, self.n_steps, self.seed, self.bridge = key, n_points, n_steps, seed, bridge

    def price(self, S_, K_, T_, r, sigma, option_type, q=0.0, **kw):
        assert K_ == K and q == Q
        return oracle_prices(self.n_steps, self.n_points, self.seed, self.bridge, S=S_, T=T_, r=r, sigma=sigma)[(*self.key, option_type)]


@pytest.mark.parametrize("kind,sub,construction", [("asian", "arithmetic", "bridge"), ("asian", "geometric", "sequential"),
                                                    ("barrier", "down-and-out", "bridge"), ("lookback", "floating", "sequential")])
def test_fused_greeks_match_the_numpy_oracle(kind, sub, construction):
    N, n, seed = 1 << 12, 40, 99
    opt, kw = _option(kind, sub, seed)
    got = compute_greeks_unified(ExoticAdapter(opt, n_paths=N, n_steps=n, method="qmc", path_construction=construction, **kw),
                                 S, K, T, R, SIG, "call", Q)
    want = compute_greeks_unified(_OraclePricer((kind, sub), N, n, seed, construction == "bridge"), S, K, T, R, SIG, "call", Q)
    assert list(got) == list(want)
    for key in want:
        assert float(got[key]) == pytest.approx(want[key], rel=1e-9, abs=1e-9), key


# -------------------------------------------------------------------------------------------------- 4. determinism ----
def test_equal_arguments_give_equal_bits_even_beside_another_context():
    def greeks(construction):
        opt, kw = _option("barrier", "up-and-in", 11)
        ad = ExoticAdapter(opt, n_paths=1 << 14, n_steps=252, method="qmc", path_construction=construction, **kw)
        return [float(v) for v in compute_greeks_unified(ad, S, K, T, R, SIG, "call", Q).values()]

    ref = {c: greeks(c) for c in ("bridge", "sequential")}
    stop, errors = threading.Event(), []

    def neighbour():     # another thread (another context): another seed, other dimension counts, other tables and bridge plans
        try:
            while not stop.is_set():
                for c, n in (("bridge", 100), ("sequential", 300), ("bridge", 37)):
                    ol.AsianOption(S, K, T, R, SIG, Q, seed=12).price(1 << 13, n, method="qmc", path_construction=c)
        except Exception as e:                      # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=neighbour)
    th.start()
    try:
        for _ in range(6):
            for c in ref:
                assert greeks(c) == ref[c]
    finally:
        stop.set()
        th.join(timeout=120)
    assert not th.is_alive()
    assert not errors, errors
