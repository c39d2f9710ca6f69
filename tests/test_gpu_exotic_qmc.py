"""Scrambled-Sobol paths for the Asian, barrier and lookback options (method="qmc"), tied to a NumPy oracle.

The oracle is written out here: SciPy's Sobol(d=n, scramble=True, seed).random(N), the clip and norm.ppf of
src/simulation/gbm_qmc.py:32-38, the sequential or Brownian-bridge construction pinned in include/olmc.h, ln S_j = ln S + j drift +
vol W_j (src/pricing_models/exotic_options.py:54-67), then the reference's payoffs on the price matrix: the Asian average
(exotic_options.py:119-130), the barrier crossing on every column t = 0..n (:200-222) and the lookback extrema (:379-401).
"""
import collections
import math
import threading
import warnings

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exotic import reference_barrier_level
from optionslab_amd.greeks import ExoticAdapter, compute_greeks_unified
from optionslab_amd.monte_carlo import sobol_tables
from tests.sobol_reference import bridge_walk, normal_chunks

pytestmark = pytest.mark.gpu

S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0
UP, DOWN = 115.0, 88.0
KINDS = [("asian", "arithmetic"), ("asian", "geometric"), ("barrier", "up-and-out"), ("barrier", "up-and-in"),
         ("barrier", "down-and-out"), ("barrier", "down-and-in"), ("lookback", "floating"), ("lookback", "fixed")]


# ----------------------------------------------------------------------------------------------------------- oracle ----
def oracle_payoffs(n, n_points, seed, bridge, mirror=False, S=S, T=T, r=R, sigma=SIG, q=Q, chunk=2048, z=None):
    """{(kind, sub, option_type): payoff vector} for Sobol points [0, n_points) (and their mirrors -z after them); with z (n_points, n)
    given, for the points whose normals are its rows."""
    dt = T / n
    drift, vol = (r - q - 0.5 * sigma**2) * dt, sigma * math.sqrt(dt)
    out = collections.defaultdict(list)
    for z in normal_chunks(n, n_points, seed, chunk, z):
        m = z.shape[0]
        for zz in ([z, -z] if mirror else [z]):
            if bridge:
                W = bridge_walk(zz)
            else:
                W = np.zeros((m, n + 1))
                W[:, 1:] = np.cumsum(zz, axis=1)
            log_S = np.empty((m, n + 1))
            log_S[:, 0] = np.log(S)
            log_S[:, 1:] = np.log(S) + np.arange(1, n + 1) * drift + vol * W[:, 1:]
            paths = np.exp(log_S)
            S_T = paths[:, -1]
            arith = np.mean(paths[:, 1:], axis=1)
            geo = np.exp(np.mean(np.log(paths[:, 1:]), axis=1))
            smax, smin = np.max(paths, axis=1), np.min(paths, axis=1)
            for ot in ("call", "put"):
                sgn = 1.0 if ot == "call" else -1.0
                out[("asian", "arithmetic", ot)].append(np.maximum(sgn * (arith - K), 0))
                out[("asian", "geometric", ot)].append(np.maximum(sgn * (geo - K), 0))
                vanilla = np.maximum(sgn * (S_T - K), 0)
                up_crossed, down_crossed = np.any(paths >= UP, axis=1), np.any(paths <= DOWN, axis=1)
                out[("barrier", "up-and-out", ot)].append(vanilla * ~up_crossed)
                out[("barrier", "up-and-in", ot)].append(vanilla * up_crossed)
                out[("barrier", "down-and-out", ot)].append(vanilla * ~down_crossed)
                out[("barrier", "down-and-in", ot)].append(vanilla * down_crossed)
                out[("lookback", "floating", ot)].append(S_T - smin if ot == "call" else smax - S_T)
                out[("lookback", "fixed", ot)].append(np.maximum(smax - K, 0) if ot == "call" else np.maximum(K - smin, 0))
    return {key: np.concatenate(v) for key, v in out.items()}


def oracle_prices(n, n_points, seed, bridge, mirror=False, **p):
    r, T_ = p.get("r", R), p.get("T", T)
    return {key: math.exp(-r * T_) * float(np.mean(v)) for key, v in oracle_payoffs(n, n_points, seed, bridge, mirror, **p).items()}


def device_price(kind, sub, option_type, n, n_points, seed, construction, antithetic=False, S_=S, T_=T, r=R, sigma=SIG):
    kw = dict(n_paths=n_points, n_steps=n, option_type=option_type, antithetic=antithetic, method="qmc", path_construction=construction)
    if kind == "asian":
        return ol.AsianOption(S_, K, T_, r, sigma, Q, seed=seed).price(avg_type=sub, **kw)
    if kind == "barrier":
        level = UP if sub.startswith("up") else DOWN
        return ol.BarrierOption(S_, K, T_, r, sigma, Q, seed=seed, barrier=level).price(barrier_type=sub, **kw)
    return ol.LookbackOption(S_, K, T_, r, sigma, Q, seed=seed).price(lookback_type=sub, **kw)


def _check_all(n, n_points, seed, construction, antithetic=False):
    want = oracle_prices(n, n_points, seed, construction == "bridge", antithetic)
    bad = []
    for kind, sub in KINDS:
        for ot in ("call", "put"):
            got = device_price(kind, sub, ot, n, n_points, seed, construction, antithetic)
            w = want[(kind, sub, ot)]
            if not got == pytest.approx(w, rel=1e-10, abs=1e-12):
                bad.append((kind, sub, ot, float(got), w))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- 1. tie to the oracle ----
@pytest.mark.parametrize("construction,n", [("bridge", n) for n in (1, 2, 3, 50, 252, 1000)]
                         + [("sequential", n) for n in (1, 2, 3, 50, 252, 1000, 4096)])
@pytest.mark.parametrize("n_points", [1, 1000, 1 << 14])
def test_qmc_paths_match_the_oracle(construction, n, n_points):
    for seed in (7, 1234, 2**31 - 5):
        _check_all(n, n_points, seed, construction)


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
@pytest.mark.parametrize("n,n_points", [(1, 1000), (3, 1000), (252, 1000), (50, 1 << 14)])
def test_qmc_antithetic_mirror_matches_the_oracle(construction, n, n_points):
    _check_all(n, n_points, 99, construction, antithetic=True)


# ------------------------------------------------------------------------------------------------- 2. shard additivity ----
@pytest.mark.parametrize("bridge", [True, False])
def test_shards_of_one_sequence_add_up(bridge):
    n, N, a = 252, 1 << 14, 4321                        # a: neither a multiple of 64 nor of 512
    sv, shift = sobol_tables(n, 5, N)
    calls = [
        lambda off, cnt: _hip.asian_qmc(S, K, T, R, SIG, Q, True, False, cnt, sv, shift, bridge, point_offset=off),
        lambda off, cnt: _hip.asian_qmc(S, K, T, R, SIG, Q, False, True, cnt, sv, shift, bridge, antithetic=True, point_offset=off),
        lambda off, cnt: _hip.extrema_qmc(S, K, T, R, SIG, Q, True, 0, reference_barrier_level(S, UP, "up-and-out"), cnt, sv, shift, bridge,
                                          point_offset=off),
        lambda off, cnt: _hip.extrema_qmc(S, K, T, R, SIG, Q, False, _hip.LOOKBACK_FLOATING, 0.0, cnt, sv, shift, bridge, point_offset=off),
    ]
    for call in calls:
        whole, lo, hi = call(0, N), call(0, a), call(a, N - a)
        assert whole.n == lo.n + hi.n
        assert whole.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12)
        assert whole.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12)


# ----------------------------------------------------------------------------------------------------- 3. determinism ----
def test_equal_seeds_give_equal_bits_even_beside_another_context():
    def price(seed, construction, kind=("asian", "arithmetic")):
        return float(device_price(kind[0], kind[1], "call", 252, 1 << 14, seed, construction))

    ref = {c: price(11, c) for c in ("bridge", "sequential")}
    assert all(price(11, c) == ref[c] for c in ref)
    other = {c: price(12, c) for c in ("bridge", "sequential")}
    # a second thread (a second context) prices another seed with other tables and another bridge plan while this one repeats seed 11
    stop, errors = threading.Event(), []

    def neighbour():
        try:
            while not stop.is_set():
                for c, n in (("bridge", 100), ("sequential", 252), ("bridge", 252)):
                    got = float(ol.AsianOption(S, K, T, R, SIG, Q, seed=12).price(1 << 14, n, method="qmc", path_construction=c))
                    if n == 252 and got != other[c]:
                        errors.append((c, got, other[c]))
        except Exception as e:                      # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=neighbour)
    th.start()
    try:
        for _ in range(10):
            for c in ref:
                assert price(11, c) == ref[c]
    finally:
        stop.set()
        th.join(timeout=120)
    assert not th.is_alive()
    assert not errors, errors


# --------------------------------------------------------------------------------------------- 4. the point of the feature ----
def _geometric_exact(n, option_type="call"):
    """The discrete geometric-average price: ln G ~ N(ln S + drift (n + 1) / 2, vol^2 sum_k ((n - k + 1) / n)^2)."""
    from scipy.stats import norm

    dt = T / n
    drift, vol = (R - Q - 0.5 * SIG**2) * dt, SIG * math.sqrt(dt)
    mu = math.log(S) + drift * (n + 1) / 2
    v = vol**2 * sum(((n - k + 1) / n) ** 2 for k in range(1, n + 1))
    sd = math.sqrt(v)
    d2 = (mu - math.log(K)) / sd
    d1 = d2 + sd
    disc = math.exp(-R * T)
    if option_type == "call":
        return disc * (math.exp(mu + v / 2) * norm.cdf(d1) - K * norm.cdf(d2))
    return disc * (K * norm.cdf(-d2) - math.exp(mu + v / 2) * norm.cdf(-d1))


def test_sobol_paths_beat_pseudo_random_paths():
    n, N, seeds = 252, 1 << 14, range(16)
    exact = _geometric_exact(n)

    def rmse(prices):
        return math.sqrt(np.mean((np.asarray(prices) - exact) ** 2))

    geo = lambda seed, **kw: float(ol.AsianOption(S, K, T, R, SIG, Q, seed=seed).price(N, n, "geometric", **kw))
    pseudo = rmse([geo(1000 + s) for s in seeds])
    bridge = rmse([geo(s, method="qmc", path_construction="bridge") for s in seeds])
    seq = rmse([geo(s, method="qmc", path_construction="sequential") for s in seeds])
    assert bridge <= pseudo / 8, (bridge, pseudo)
    assert seq <= pseudo / 3, (seq, pseudo)

    look = lambda seed, **kw: float(ol.LookbackOption(S, K, T, R, SIG, Q, seed=seed).price(N, n, "floating", **kw))
    sd_pseudo = float(np.std([look(1000 + s) for s in seeds], ddof=1))
    sd_bridge = float(np.std([look(s, method="qmc") for s in seeds], ddof=1))
    assert sd_bridge <= sd_pseudo / 5, (sd_bridge, sd_pseudo)


# ---------------------------------------------------------------------------------------------------------- 5. Greeks ----
class _OraclePricer:
    """compute_greeks_unified's pricer protocol over the oracle (arithmetic Asian call on the bridge)."""

    def __init__(self, n_points, n_steps, seed):
        self.n_points, self.n_steps, self.seed = n_points, n_steps, seed

    def price(self, S_, K_, T_, r, sigma, option_type, q=0.0, **kw):
        assert K_ == K and q == Q
        return oracle_prices(self.n_steps, self.n_points, self.seed, True, S=S_, T=T_, r=r, sigma=sigma)[("asian", "arithmetic", option_type)]


def test_qmc_greeks_through_the_exotic_adapter_match_the_oracle():
    N, n, seed = 1 << 14, 64, 321
    asian = ol.AsianOption(S, K, T, R, SIG, Q, seed=seed)
    got = compute_greeks_unified(ExoticAdapter(asian, method="qmc", n_paths=N, n_steps=n), S, K, T, R, SIG, "call", Q)
    want = compute_greeks_unified(_OraclePricer(N, n, seed), S, K, T, R, SIG, "call", Q)
    assert list(got) == list(want)
    for key in want:
        assert float(got[key]) == pytest.approx(want[key], rel=1e-9, abs=1e-9), key
