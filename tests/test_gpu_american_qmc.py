"""The American option (LSM) and its exercise boundary on scrambled-Sobol paths (method="qmc"), tied to a NumPy oracle.

The oracle is written out here: SciPy's Sobol(d=n, scramble=True, seed).random(N), the clip and norm.ppf of
src/simulation/gbm_qmc.py:32-38, the pinned Brownian bridge or a cumulative sum (include/olmc.h), ln S_j = ln S + j drift + vol W_j
and exp.  The regression and the boundary are the reference's algorithm (oracle/numpy_reference.py american_from_paths,
exercise_boundary_from_paths), applied to the device's own exported matrix and to the SciPy-built one.
"""
import collections
import math
import threading
import warnings

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from optionslab_amd.greeks import ExoticAdapter, compute_greeks_unified
from optionslab_amd.monte_carlo import sobol_tables
from oracle import numpy_reference as orc
from tests.sobol_reference import bridge_walk, normal_chunks

pytestmark = pytest.mark.gpu

T, R = 1.0, 0.05


# ----------------------------------------------------------------------------------------------------------- oracle ----
def oracle_paths(S, T_, r, sigma, q, n, n_points, seed, bridge, chunk=4096, z=None):
    """Yields (row0, prices (m, n + 1)) over Sobol points [0, n_points) in chunks; column 0 = S.  With z (n_points, n) given, over the
    points whose normals are its rows."""
    dt = T_ / n
    drift, vol = (r - q - 0.5 * sigma**2) * dt, sigma * math.sqrt(dt)
    done = 0
    for z in normal_chunks(n, n_points, seed, chunk, z):
        m = z.shape[0]
        if bridge:
            W = bridge_walk(z)
        else:
            W = np.zeros((m, n + 1))
            W[:, 1:] = np.cumsum(z, axis=1)
        log_S = np.empty((m, n + 1))
        log_S[:, 0] = np.log(S)
        log_S[:, 1:] = np.log(S) + np.arange(1, n + 1) * drift + vol * W[:, 1:]
        p = np.exp(log_S)
        p[:, 0] = S
        yield done, p
        done += m


def reference_column0(S, n):
    """exotic_options.py:64-67: the reference's column 0 is np.exp(np.log(S))."""
    return np.exp(np.full(n, np.log(S)))


def device_paths(S, T_, r, sigma, q, n, n_points, seed, bridge):
    sv, shift = sobol_tables(n, seed, n_points)
    return _hip.gbm_qmc_paths(S, T_, r, sigma, q, n_points, sv, shift, bridge, path_major=True)


def tied_paths(S, T_, r, sigma, q, n, n_points, seed, bridge):
    """The device's matrix, column 0 as the reference's (what the LSM chain and the boundary read)."""
    p = device_paths(S, T_, r, sigma, q, n, n_points, seed, bridge)
    p[:, 0] = reference_column0(S, n_points)
    return p


# ------------------------------------------------------------------------------------- 1. the matrix against the oracle ----
@pytest.mark.parametrize("construction,n", [("bridge", n) for n in (1, 2, 3, 50, 252, 1000)]
                         + [("sequential", n) for n in (1, 50, 1000, 4096)])
@pytest.mark.parametrize("n_points", [1, 1000, 4097, 1 << 14])
def test_the_path_matrix_matches_the_oracle(construction, n, n_points):
    S, sigma, q = 100.0, 0.25, 0.01
    bridge = construction == "bridge"
    for seed in (7, 1234, 2**31 - 5):
        sv, shift = sobol_tables(n, seed, n_points)
        pm = _hip.gbm_qmc_paths(S, T, R, sigma, q, n_points, sv, shift, bridge, path_major=True)
        tm = _hip.gbm_qmc_paths(S, T, R, sigma, q, n_points, sv, shift, bridge, path_major=False)
        assert pm.shape == (n_points, n + 1) and tm.shape == (n + 1, n_points)
        assert np.array_equal(pm, tm.T)                                     # bit for bit: the same arithmetic in both layouts
        assert np.all(pm[:, 0] == S)
        for row0, want in oracle_paths(S, T, R, sigma, q, n, n_points, seed, bridge):
            got = pm[row0:row0 + want.shape[0]]
            err = np.max(np.abs(got - want) / want)
            assert err <= 1e-12, (construction, n, n_points, seed, row0, err)
        del pm, tm


def test_the_public_export_is_the_device_matrix():
    got = ol.simulate_gbm_qmc_paths_hip(100.0, T, R, 0.2, 0.0, 1000, 50, 11)
    assert np.array_equal(got, device_paths(100.0, T, R, 0.2, 0.0, 50, 1000, 11, True))
    seq = ol.simulate_gbm_qmc_paths_hip(100.0, T, R, 0.2, 0.0, 1000, 50, 11, path_construction="sequential")
    assert np.array_equal(seq, device_paths(100.0, T, R, 0.2, 0.0, 50, 1000, 11, False))


# -------------------------------------------------------------------------------- 2. the price, tied per scramble ----
AMERICAN_TIE = 1e-9
AMERICAN_TIE_DEGREE_4 = 1e-3
CASES = [
    (100.0, 100.0, 0.2, 0.0, False, 50_000, 50, 3), (90.0, 100.0, 0.3, 0.0, False, 20_001, 25, 2),
    (100.0, 110.0, 0.25, 0.0, False, 30_000, 52, 1), (95.0, 100.0, 0.15, 0.0, False, 20_000, 13, 3),
    (100.0, 100.0, 0.2, 0.08, True, 20_000, 40, 3), (110.0, 100.0, 0.3, 0.06, True, 10_007, 33, 2),
    (100.0, 90.0, 0.25, 0.05, True, 15_000, 21, 1), (100.0, 100.0, 0.2, 0.0, False, 5_000, 1, 3),
    (100.0, 95.0, 0.25, 0.0, False, 20_000, 13, 4), (100.0, 100.0, 0.4, 0.0, False, 40_000, 6, 4),
]
SEED = 7


def assert_tied(st, price, x, rel):
    assert st.n == len(x)
    assert st.sum == pytest.approx(float(np.sum(x)), rel=rel, abs=1e-300)
    assert st.sumsq == pytest.approx(float(np.sum(x * x)), rel=2 * rel, abs=1e-300)
    assert st.price == pytest.approx(float(price), rel=rel, abs=1e-300)


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
@pytest.mark.parametrize("S,K,v,q,call,N,M,deg", CASES)
def test_american_qmc_tied_to_the_reference_algorithm(construction, S, K, v, q, call, N, M, deg):
    bridge = construction == "bridge"
    sv, shift = sobol_tables(M, SEED, N)
    st = _hip.american_lsm_qmc(S, K, T, R, v, q, call, N, sv, shift, bridge, deg)
    typ = "call" if call else "put"
    price, x = orc.american_from_paths(tied_paths(S, T, R, v, q, M, N, SEED, bridge), K, T, R, typ, deg, return_payoffs=True)
    rel = AMERICAN_TIE_DEGREE_4 if deg == 4 else AMERICAN_TIE
    assert_tied(st, price, x, rel)
    # the same price through the public method
    got = ol.AmericanOption(S, K, T, R, v, q, seed=SEED).price(N, M, typ, deg, method="qmc", path_construction=construction)
    assert float(got) == st.price
    if deg <= 3:                                    # and on the matrix SciPy itself builds (well-conditioned cases)
        want = np.concatenate([p for _, p in oracle_paths(S, T, R, v, q, M, N, SEED, bridge)])
        want[:, 0] = reference_column0(S, N)
        assert st.price == pytest.approx(float(orc.american_from_paths(want, K, T, R, typ, deg)), rel=AMERICAN_TIE, abs=1e-300)


# -------------------------------------------------------------------------------------------------- 3. the boundary ----
@pytest.mark.parametrize("construction", ["bridge", "sequential"])
@pytest.mark.parametrize("S,K,v,q,typ,N,M", [
    (100.0, 100.0, 0.2, 0.0, "put", 10_000, 50), (100.0, 100.0, 0.2, 0.05, "call", 4_097, 33),
    (100.0, 60.0, 0.2, 0.0, "put", 300_000, 6),            # few in the money, none at the first dates: NaN
    (100.0, 1.0, 0.1, 0.0, "put", 1_000, 4),               # nobody in the money at any date
])
def test_boundary_tied_to_the_reference_algorithm(construction, S, K, v, q, typ, N, M):
    times, b = ol.AmericanOption(S, K, T, R, v, q, seed=SEED).early_exercise_boundary(N, M, typ, method="qmc", path_construction=construction)
    assert np.array_equal(times, np.linspace(0, T, M + 1)) and b.shape == (M + 1,)
    want = orc.exercise_boundary_from_paths(tied_paths(S, T, R, v, q, M, N, SEED, construction == "bridge"), K, typ)
    # exact: NumPy's percentile of the very paths the device selected from.  Date 0 compares exp(ln S) with K on each side's own
    # exponential (libm's and NumPy's may differ by an ulp there), as in tests/test_gpu_exotics.py
    assert np.array_equal(b[1:], want[1:], equal_nan=True)
    assert np.isnan(b[0]) or b[0] == pytest.approx(S, rel=1e-14)
    if K == 1.0:
        assert np.all(np.isnan(b))


# ------------------------------------------------------------------------------------------ 4. the point of the feature ----
def bermudan_tree(S, K, T_, r, v, dates, sub=40):
    """A CRR tree of the put that allows exercise on the same dates (sub tree steps between dates)."""
    n = dates * sub
    dt = T_ / n
    u = math.exp(v * math.sqrt(dt))
    p = (math.exp(r * dt) - 1 / u) / (u - 1 / u)
    disc = math.exp(-r * dt)
    j = np.arange(n + 1)
    val = np.maximum(K - S * u ** (2.0 * j - n), 0.0)
    for i in range(n - 1, -1, -1):
        val = disc * (p * val[1:] + (1 - p) * val[:-1])
        if i % sub == 0 and i > 0:
            val = np.maximum(val, K - S * u ** (2.0 * np.arange(i + 1) - i))
    return float(val[0])


def test_bridge_sobol_paths_shrink_the_spread_of_the_american_price():
    S, K, v, N, n = 100.0, 100.0, 0.2, 1 << 14, 50
    tree = bermudan_tree(S, K, T, R, v, n)
    assert 6.07 < tree < 6.09
    pseudo = np.array([float(ol.AmericanOption(S, K, T, R, v, seed=1000 + s).price(N, n, "put", 3)) for s in range(16)])
    bridge = np.array([float(ol.AmericanOption(S, K, T, R, v, seed=s).price(N, n, "put", 3, method="qmc")) for s in range(16)])
    sd_pseudo, sd_bridge = float(np.std(pseudo, ddof=1)), float(np.std(bridge, ddof=1))
    assert sd_bridge <= sd_pseudo / 2.5, (sd_bridge, sd_pseudo)
    # both means within 3 standard errors of the tree.  LSM's in-sample bias (~1e-2 here, tests/test_gpu_exotics.py allows it too) is
    # 3 standard errors of the pseudo-random mean at this size (the CPU oracle on NumPy normals: 6.106 against 6.078, se 0.009), so the
    # Philox mean gets that allowance; on the bridge it is below one standard error (oracle: 6.083, se 0.003)
    for prices, allowance in ((pseudo, 0.01), (bridge, 0.0)):
        se = float(np.std(prices, ddof=1)) / math.sqrt(len(prices))
        assert abs(float(np.mean(prices)) - tree) <= 3 * se + allowance, (float(np.mean(prices)), tree, se)


# ------------------------------------------------------------------------------------- 5. determinism and isolation ----
def test_equal_seeds_give_equal_bits_beside_a_philox_american():
    S, K, v, N, n = 100.0, 100.0, 0.2, 1 << 14, 50
    qmc = lambda c: float(ol.AmericanOption(S, K, T, R, v, seed=11).price(N, n, method="qmc", path_construction=c))
    philox = lambda: float(ol.AmericanOption(S, K, T, R, v, seed=12).price(N, n))
    ref = {c: qmc(c) for c in ("bridge", "sequential")}
    philox_ref = philox()
    stop, errors = threading.Event(), []

    def neighbour():
        try:
            while not stop.is_set():
                got = philox()
                if got != philox_ref:
                    errors.append(("philox", got, philox_ref))
        except Exception as e:                      # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=neighbour)
    th.start()
    try:
        for _ in range(10):
            for c in ref:
                assert qmc(c) == ref[c]
    finally:
        stop.set()
        th.join(timeout=120)
    assert not th.is_alive()
    assert not errors, errors


def test_a_qmc_call_leaves_the_philox_american_unchanged():
    opt = ol.AmericanOption(100.0, 100.0, T, R, 0.2, seed=5)
    before = float(opt.price(20_000, 50))
    b_before = opt.early_exercise_boundary(10_000, 50)[1]
    opt.price(20_000, 50, method="qmc")
    opt.early_exercise_boundary(10_000, 50, method="qmc")
    assert float(opt.price(20_000, 50)) == before
    assert np.array_equal(opt.early_exercise_boundary(10_000, 50)[1], b_before, equal_nan=True)


def test_a_million_points_by_fifty_dates():
    for c in ("bridge", "sequential"):
        price, se = ol.AmericanOption(100.0, 100.0, T, R, 0.2, seed=3).price(1 << 20, 50, return_error=True, method="qmc", path_construction=c)
        assert math.isfinite(price) and 5.9 < price < 6.2 and se > 0


def test_a_matrix_over_64_gb_is_refused():
    sv, shift = sobol_tables(8, 3, 1 << 30)
    with pytest.raises(AccelerationError, match="64 GB"):
        _hip.american_lsm_qmc(100.0, 100.0, T, R, 0.2, 0.0, False, 1 << 30, sv, shift, True, 3)
    # and the context is still usable
    assert math.isfinite(float(ol.AmericanOption(100.0, 100.0, T, R, 0.2, seed=3).price(1000, 8, method="qmc")))


# ---------------------------------------------------------------------------------------------------------- 6. Greeks ----
class _LiteralPricer:
    """compute_greeks_unified's pricer protocol over AmericanOption.price(method="qmc") itself, one pricing per bump."""

    def __init__(self, n_points, n_steps, seed):
        self.n_points, self.n_steps, self.seed = n_points, n_steps, seed

    def price(self, S_, K_, T_, r, sigma, option_type, q=0.0, **kw):
        return ol.AmericanOption(S_, K_, T_, r, sigma, q, seed=self.seed).price(self.n_points, self.n_steps, option_type, method="qmc")


def test_qmc_greeks_through_the_exotic_adapter():
    S, K, v, N, n, seed = 100.0, 100.0, 0.2, 1 << 14, 50, 321
    adapter = ExoticAdapter(ol.AmericanOption(S, K, T, R, v, seed=seed), method="qmc", n_paths=N, n_steps=n)
    got = compute_greeks_unified(adapter, S, K, T, R, v, "put")
    want = compute_greeks_unified(_LiteralPricer(N, n, seed), S, K, T, R, v, "put")
    assert list(got) == list(want)
    for key in want:
        assert math.isfinite(float(got[key])), key
        assert float(got[key]) == float(want[key]), key
    assert -1.0 < float(got["delta"]) < 0.0
