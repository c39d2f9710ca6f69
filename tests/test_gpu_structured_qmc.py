"""Scrambled-Sobol paths for the autocallable and the cliquet (method="qmc"), tied to a NumPy oracle.

The oracle is written out here: SciPy's Sobol(d=n, scramble=True, seed).random(N), the clip and norm.ppf of
src/simulation/gbm_qmc.py:32-38, the sequential or Brownian-bridge construction pinned in include/olmc.h, ln S_j = ln S + j drift +
vol W_j (src/pricing_models/exotic_options.py:54-67), then the reference-pinned payoffs on the price matrix,
oracle.numpy_reference.autocallable_from_paths / cliquet_from_paths.  The mirror is the same on -z, its payoffs after the first N.

The ties are exact (every path counts): over all the autocallable cases of test 1 at N = 2^14, both constructions and both legs, the
smallest distance in log units between an observed S_t / S and the autocall level, the path minimum and the knock-in level, S_T / S
and the coupon level or 1 is 3.0e-8 on the oracle alone, five orders above the arithmetic's 1e-13; the cliquet payoff is continuous.
"""
import collections
import math
import threading
import warnings

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.greeks import ExoticAdapter, compute_greeks_unified
from optionslab_amd.monte_carlo import sobol_tables
from oracle import numpy_reference as ref
from tests.sobol_reference import bridge_walk, normal_chunks

pytestmark = pytest.mark.gpu

S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0
SEEDS = (7, 1234, 2**31 - 5)
COUNTS = (1, 1000, 1 << 14)
AUTO_DEFAULTS = dict(autocall_barrier=1.0, coupon_barrier=0.8, coupon_rate=0.10, ki_barrier=0.6)
CLIQ_DEFAULTS = dict(local_cap=0.05, local_floor=-0.05, global_cap=0.30, global_floor=0.0)

# (n, observation_freq, overrides); the bridge takes at most 1024 dates
AUTO_CASES = [
    (252, 21, {}),
    (100, 30, dict(autocall_barrier=1.05, ki_barrier=0.9)),        # 10 trailing dates
    (13, 13, dict(autocall_barrier=1.02)),                         # one observation, at maturity
    (252, 63, dict(autocall_barrier=1.15)),
    (1000, 50, {}),
    (64, 1, dict(autocall_barrier=1.1, ki_barrier=0.8)),           # every date observed
    (3, 2, {}),
    (4096, 256, {}),                                               # sequential only
]
# (n, n_periods, overrides)
CLIQ_CASES = [
    (252, 12, {}),
    (100, 7, {}),                                                  # 2 trailing dates
    (13, 13, {}),                                                  # one-date periods
    (64, 1, {}),
    (1000, 12, {}),                                                # 83-date periods: reset dates cross the 64-lane trips
    (1, 1, {}),
    (252, 4, dict(local_cap=0.10, local_floor=-0.10, global_cap=1.0, global_floor=-1.0)),
    (4096, 5, {}),                                                 # sequential only
]


def constructions(n):
    return ("bridge", "sequential") if n <= 1024 else ("sequential",)


# ----------------------------------------------------------------------------------------------------------- oracle ----
def oracle_paths(n, n_points, seed, S=S, T=T, r=R, sigma=SIG, q=Q, chunk=2048, z=None):
    """Yields {(construction, leg): price matrix (m, n + 1)} for consecutive chunks of Sobol points [0, n_points); leg 1 is the mirror -z.
    With z (n_points, n) given, for the points whose normals are its rows."""
    dt = T / n
    drift, vol = (r - q - 0.5 * sigma**2) * dt, sigma * math.sqrt(dt)
    for z in normal_chunks(n, n_points, seed, chunk, z):
        m = z.shape[0]
        out = {}
        for construction in constructions(n):
            for leg, zz in enumerate((z, -z)):
                if construction == "bridge":
                    W = bridge_walk(zz)
                else:
                    W = np.zeros((m, n + 1))
                    W[:, 1:] = np.cumsum(zz, axis=1)
                log_S = np.empty((m, n + 1))
                log_S[:, 0] = np.log(S)
                log_S[:, 1:] = np.log(S) + np.arange(1, n + 1) * drift + vol * W[:, 1:]
                out[(construction, leg)] = np.exp(log_S)
        yield out


def auto_payoffs(paths, f, over, S_=S, T_=T, r=R):
    return ref.autocallable_from_paths(paths, S_, T_, r, f, **{**AUTO_DEFAULTS, **over}, return_payoffs=True)[1]


def cliq_payoffs(paths, periods, over, S_=S, T_=T, r=R):
    return ref.cliquet_from_paths(paths, S_, T_, r, periods, **{**CLIQ_DEFAULTS, **over}, return_payoffs=True)[1]


def oracle_vectors(n, n_points, seed, jobs, **market):
    """{(job index, construction, leg): payoff vector over points [0, n_points)}; a job is (payoff function, parameter, overrides).
    z=(n_points, n) normals among the keywords: the points whose normals are its rows."""
    parts = collections.defaultdict(list)
    p = {k_: market[k_] for k_ in ("S", "T", "r") if k_ in market}
    kw = dict(S_=p.get("S", S), T_=p.get("T", T), r=p.get("r", R))
    for chunk in oracle_paths(n, n_points, seed, **market):
        for (construction, leg), paths in chunk.items():
            for i, (fn, par, over) in enumerate(jobs):
                parts[(i, construction, leg)].append(fn(paths, par, over, **kw))
    return {key: np.concatenate(v) for key, v in parts.items()}


def device_stats(product, par, over, n, n_points, seed, construction, antithetic=False, point_offset=0, S_=S, T_=T, r=R, sigma=SIG):
    sv, shift = sobol_tables(n, seed, point_offset + n_points)
    bridge = construction == "bridge"
    if product == "auto":
        a = {**AUTO_DEFAULTS, **over}
        return _hip.autocallable_qmc(S_, T_, r, sigma, Q, a["autocall_barrier"], a["coupon_barrier"], a["coupon_rate"], a["ki_barrier"], par,
                                     n_points, sv, shift, bridge, antithetic, point_offset)
    c = {**CLIQ_DEFAULTS, **over}
    return _hip.cliquet_qmc(S_, T_, r, sigma, Q, c["local_cap"], c["local_floor"], c["global_cap"], c["global_floor"], par, n_points, sv, shift,
                            bridge, antithetic, point_offset)


def option_of(product, over, seed, S_=S, T_=T, r=R, sigma=SIG):
    if product == "auto":
        return ol.AutocallableOption(S_, K, T_, r, sigma, Q, seed=seed, **{**AUTO_DEFAULTS, **over})
    return ol.CliquetOption(S_, K, T_, r, sigma, Q, seed=seed, **{**CLIQ_DEFAULTS, **over})


def class_price(product, par, over, n, n_points, seed, **kw):
    name = "observation_freq" if product == "auto" else "n_periods"
    return float(option_of(product, over, seed).price(n_points, n, **{name: par}, **kw))


def _price_of(product, x, r=R, T_=T):
    return float(np.mean(x)) if product == "auto" else math.exp(-r * T_) * float(np.mean(x))     # the autocallable's payoffs carry their discount


# ------------------------------------------------------------------------------------------------- 1. tie to the oracle ----
def _tie(product, n, jobs):
    fn = auto_payoffs if product == "auto" else cliq_payoffs
    bad = []
    for seed in SEEDS:
        want = oracle_vectors(n, max(COUNTS), seed, [(fn, par, over) for par, over in jobs])
        for i, (par, over) in enumerate(jobs):
            for construction in constructions(n):
                for count in COUNTS:
                    for antithetic in (False, True):
                        x = np.concatenate([want[(i, construction, leg)][:count] for leg in ((0, 1) if antithetic else (0,))])
                        st = device_stats(product, par, over, n, count, seed, construction, antithetic)
                        price = _price_of(product, x)
                        figures = (seed, par, construction, count, antithetic, st.price, price, st.sum, float(np.sum(x)))
                        print(product, n, *figures)
                        ok = (st.n == len(x) and st.price == pytest.approx(price, rel=1e-10, abs=1e-12)
                              and st.sum == pytest.approx(float(np.sum(x)), rel=1e-10, abs=1e-12)
                              and st.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10, abs=1e-12))
                        if not ok:
                            bad.append(figures + (st.n, st.sumsq, float(np.sum(x * x))))
    assert not bad, bad


def _by_n(cases):
    groups = collections.OrderedDict()
    for n, par, over in cases:
        groups.setdefault(n, []).append((par, over))
    return list(groups.items())


@pytest.mark.parametrize("n,jobs", _by_n(AUTO_CASES), ids=[f"n{n}" for n, _ in _by_n(AUTO_CASES)])
def test_autocallable_on_sobol_paths_matches_the_oracle(n, jobs):
    _tie("auto", n, jobs)


@pytest.mark.parametrize("n,jobs", _by_n(CLIQ_CASES), ids=[f"n{n}" for n, _ in _by_n(CLIQ_CASES)])
def test_cliquet_on_sobol_paths_matches_the_oracle(n, jobs):
    _tie("cliq", n, jobs)


def test_the_classes_price_what_the_bindings_price_and_an_autocallable_without_an_observation_date():
    # through the classes: (8, 21, -) has no observation date (range(21, 9, 21) is empty: every path runs to maturity)
    n, count = 8, 1 << 14
    for seed in SEEDS:
        want = oracle_vectors(n, count, seed, [(auto_payoffs, 21, {}), (cliq_payoffs, 4, {})])
        for construction in constructions(n):
            for antithetic in (False, True):
                legs = (0, 1) if antithetic else (0,)
                for i, (product, par) in enumerate((("auto", 21), ("cliq", 4))):
                    x = np.concatenate([want[(i, construction, leg)] for leg in legs])
                    got = class_price(product, par, {}, n, count, seed, method="qmc", path_construction=construction, antithetic=antithetic)
                    assert got == pytest.approx(_price_of(product, x), rel=1e-10, abs=1e-12), (product, seed, construction, antithetic)
    # return_error: the naive per-path standard error of the payoffs (ddof = 0, as every olmc_stats), the price's discount on it
    x = want[(1, "sequential", 0)]
    price, err = option_of("cliq", {}, SEEDS[-1]).price(count, n, n_periods=4, method="qmc", path_construction="sequential", return_error=True)
    assert float(price) == pytest.approx(_price_of("cliq", x), rel=1e-10)
    assert err == pytest.approx(math.exp(-R * T) * float(np.std(x)) / math.sqrt(count), rel=1e-6)


# --------------------------------------------------------------------------------- 2. tie to the device's own Sobol matrix ----
@pytest.mark.parametrize("product,n,par,over,construction,count", [
    ("auto", 252, 21, {}, "bridge", 1 << 14),
    ("auto", 100, 30, dict(autocall_barrier=1.05, ki_barrier=0.9), "sequential", 1000),
    ("cliq", 252, 12, {}, "bridge", 1 << 14),
    ("cliq", 1000, 12, {}, "sequential", 1000),
])
def test_the_payoffs_on_the_devices_own_sobol_matrix(product, n, par, over, construction, count):
    seed = 1234
    sv, shift = sobol_tables(n, seed, count)
    paths = np.array(_hip.gbm_qmc_paths(S, T, R, SIG, Q, count, sv, shift, construction == "bridge", path_major=True)).reshape(count, n + 1)
    paths[:, 0] = np.exp(np.log(S))
    x = (auto_payoffs if product == "auto" else cliq_payoffs)(paths, par, over)
    st = device_stats(product, par, over, n, count, seed, construction)
    # the matrix sums W in another association (include/olmc.h "quasi-Monte Carlo path matrix"): a few ulps
    assert st.price == pytest.approx(_price_of(product, x), rel=1e-9)


# ------------------------------------------------------------------------------------------------- 3. shard additivity ----
@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_shards_of_one_sequence_add_up(construction):
    n, N, a = 252, 1 << 14, 4321                        # a: neither a multiple of 64 nor of 512
    for product, par, antithetic in (("auto", 21, False), ("auto", 63, True), ("cliq", 12, False), ("cliq", 4, True)):
        call = lambda off, cnt: device_stats(product, par, {}, n, cnt, 5, construction, antithetic, point_offset=off)
        whole, lo, hi = call(0, N), call(0, a), call(a, N - a)
        assert whole.n == lo.n + hi.n
        assert whole.sum == pytest.approx(lo.sum + hi.sum, rel=1e-12)
        assert whole.sumsq == pytest.approx(lo.sumsq + hi.sumsq, rel=1e-12)


# ----------------------------------------------------------------------------------------------------- 4. determinism ----
def test_equal_seeds_give_equal_bits_even_beside_another_context():
    jobs = [(p, par, c) for p, par in (("auto", 21), ("cliq", 12)) for c in ("bridge", "sequential")]

    def price(seed, job, n=252):
        product, par, construction = job
        return class_price(product, par, {}, n, 1 << 14, seed, method="qmc", path_construction=construction)

    ref_bits = {job: price(11, job) for job in jobs}
    assert all(price(11, job) == ref_bits[job] for job in jobs)
    other = {job: price(12, job) for job in jobs}
    # a second thread (a second context) prices another seed with other tables and another bridge plan while this one repeats seed 11
    stop, errors = threading.Event(), []

    def neighbour():
        try:
            while not stop.is_set():
                for job in jobs:
                    price(12, job, 100)
                    got = price(12, job)
                    if got != other[job]:
                        errors.append((job, got, other[job]))
        except Exception as e:                      # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=neighbour)
    th.start()
    try:
        for _ in range(10):
            for job in jobs:
                assert price(11, job) == ref_bits[job]
    finally:
        stop.set()
        th.join(timeout=120)
    assert not th.is_alive()
    assert not errors, errors


# ------------------------------------------------------------------------------------------- 5. method="pseudo" is untouched ----
def test_pseudo_is_bit_for_bit_what_it_was():
    N, n, seed = 1 << 14, 252, 77
    auto, cliq = option_of("auto", {}, seed), option_of("cliq", {}, seed)
    want_a = _hip.autocallable(S, T, R, SIG, Q, 1.0, 0.8, 0.10, 0.6, 21, N, n, seed, False).price
    want_c = _hip.cliquet(S, T, R, SIG, Q, 0.05, -0.05, 0.30, 0.0, 12, N, n, seed, True).price
    for kw in (dict(), dict(method="pseudo"), dict(method="pseudo", path_construction="sequential")):
        assert float(auto.price(N, n, **kw)) == want_a
        assert float(cliq.price(N, n, antithetic=True, **kw)) == want_c


# --------------------------------------------------------------------------------------------- 6. the point of the feature ----
@pytest.mark.parametrize("product,par,over,factor", [
    ("auto", 21, {}, 1.5),
    ("auto", 21, dict(autocall_barrier=1.05, ki_barrier=0.8), 1.5),
    ("cliq", 12, {}, 2.0),
    ("cliq", 4, dict(local_cap=0.10, local_floor=-0.10, global_cap=1.0, global_floor=-1.0), 15.0),
])
def test_sobol_paths_beat_pseudo_random_paths(product, par, over, factor):
    # the bounds are the CPU oracle's measured ratios of standard deviations (2.2, 2.8, 3.6, 42) with room for the scatter of a
    # 16-sample standard deviation (about +-25 % each side of the ratio); the device prices the same points to 1e-10
    n, N, seeds = 252, 1 << 14, range(16)
    sd_pseudo = float(np.std([class_price(product, par, over, n, N, 1000 + s) for s in seeds], ddof=1))
    sd_bridge = float(np.std([class_price(product, par, over, n, N, s, method="qmc") for s in seeds], ddof=1))
    print(product, par, over, "pseudo", sd_pseudo, "bridge", sd_bridge, "ratio", sd_pseudo / sd_bridge)
    assert sd_bridge <= sd_pseudo / factor, (sd_bridge, sd_pseudo)


# ---------------------------------------------------------------------------------------------------------- 7. Greeks ----
class _OraclePricer:
    """compute_greeks_unified's pricer protocol over the oracle (bridge construction)."""

    def __init__(self, product, par, n_points, n_steps, seed):
        self.product, self.par, self.n_points, self.n_steps, self.seed = product, par, n_points, n_steps, seed

    def price(self, S_, K_, T_, r, sigma, option_type, q=0.0, **kw):
        assert K_ == K and q == Q
        fn = auto_payoffs if self.product == "auto" else cliq_payoffs
        x = oracle_vectors(self.n_steps, self.n_points, self.seed, [(fn, self.par, {})], S=S_, T=T_, r=r, sigma=sigma)[(0, "bridge", 0)]
        return _price_of(self.product, x, r, T_)


def test_qmc_greeks_through_the_exotic_adapter_match_the_oracle():
    N, n, seed = 1 << 14, 64, 321
    cliq = option_of("cliq", {}, seed)
    got = compute_greeks_unified(ExoticAdapter(cliq, method="qmc", n_paths=N, n_steps=n, n_periods=12), S, K, T, R, SIG, "call", Q)
    want = compute_greeks_unified(_OraclePricer("cliq", 12, N, n, seed), S, K, T, R, SIG, "call", Q)
    assert list(got) == list(want)
    for key in want:
        assert float(got[key]) == pytest.approx(want[key], rel=1e-9, abs=1e-9), key

    # the autocallable's levels are relative to spot: the spot bumps price the same contract.  Its bumped contracts (sigma, r, T) stay
    # as far from every decision as the cases of test 1: the smallest distance over the evaluations of this call, measured on the
    # oracle as described at the top of this file, is 6.6e-8 log units.
    auto = option_of("auto", {}, seed)
    got = compute_greeks_unified(ExoticAdapter(auto, method="qmc", n_paths=N, n_steps=n, observation_freq=21), S, K, T, R, SIG, "call", Q)
    want = compute_greeks_unified(_OraclePricer("auto", 21, N, n, seed), S, K, T, R, SIG, "call", Q)
    assert list(got) == list(want)
    assert abs(float(got["delta"])) <= 1e-9 and abs(float(got["gamma"])) <= 1e-9
    for key in ("price", "vega", "rho", "theta"):
        assert float(got[key]) == pytest.approx(want[key], rel=1e-9, abs=1e-9), key
