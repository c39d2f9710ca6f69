"""Per-seed tie of the path-dependent kernels to the REFERENCE's payoff algorithm (oracle/numpy_reference.py, pinned `==` to the
reference by tests/test_oracle_golden.py), not to the build's own C restatement of the device (tests/test_gpu_exotics.py).

Every case draws the device's own path matrix (olmc_gbm_paths: the same Philox stream, raw normals and fp64 fma(vol, z, drift)
recursion as the Asian, barrier / lookback, autocallable and LSM kernels), puts the reference's np.exp(np.log(S)) in column 0
(exotic_options.py:64-67; olmc_gbm_paths stores S there, as simulate_gbm_paths does), applies the oracle's *_from_paths in fp64 and
compares n, sum, sumsq and price with the kernel's olmc_stats on the same seed.  A monitoring-date, observation-index, t = 0 or clip
convention that is off moves these by far more than the tolerances, which follow from the kernels' arithmetic:
  EXACT  fp64 on bit-identical cumulative log-returns (barrier, lookback, autocallable, arithmetic Asian, American): only the
         exponential's last bits and the order of the final sums differ;
  REL    fp32 partial sums of the normals or of the log-prices (geometric and fast arithmetic Asian, cliquet): the checker's 2e-6.
The reference has no antithetic mirror: for antithetic=True the mirrored leg is rebuilt on the host from the device paths'
log-increments as 2 drift - increment, and the two legs are tied together.
The device's own matrix is itself pinned in tests/test_gpu_path_matrices_exact.py: to a long-double recursion on the stream's draws,
within (t + 8) M 2^-52 on ln S."""
import math

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exotic import reference_barrier_level
from oracle import numpy_reference as orc

pytestmark = pytest.mark.gpu
EXACT = 1e-12
REL = 2e-6
# the mirrored leg goes through log() of the device prices and a cumulative sum of the recovered increments: ~1e-16 per date
# relative on the rebuilt prices, a few 1e-14 after 252 dates -- still five orders below any convention error
MIRROR = 1e-10
T, R, V, Q = 1.0, 0.05, 0.2, 0.01
SEED = 7


def reference_column0(S, n):
    """exotic_options.py:64-67: log_S[:, 0] = np.log(S); paths = np.exp(log_S) -- the array exponential, as the reference takes it."""
    return np.exp(np.full(n, np.log(S)))


def tied_paths(S, N, M, seed, antithetic=False, T=T, r=R, v=V, q=Q):
    """The device's path matrix, column 0 as the reference's; with antithetic the mirrored rows follow the first N."""
    p = _hip.gbm_paths(S, T, r, v, q, N, M, seed, path_major=True)
    assert p.shape == (N, M + 1) and np.all(p[:, 0] == S)
    if antithetic:
        drift = (r - q - 0.5 * v * v) * (T / M)                     # the host's per-step drift (exotic_options.py:54-56)
        log_p = np.log(p)
        inc = np.diff(log_p, axis=1)
        mirror = np.empty_like(p)
        mirror[:, 0] = S
        mirror[:, 1:] = np.exp(log_p[:, :1] + np.cumsum(2.0 * drift - inc, axis=1))
        p = np.concatenate([p, mirror])
    p[:, 0] = reference_column0(S, p.shape[0])
    return p


def assert_tied(st, price, x, rel, disc=1.0):
    """olmc_stats against the oracle's price and per-path values x (st.sum / st.sumsq are of x, undiscounted)."""
    assert st.n == len(x)
    assert st.sum == pytest.approx(float(np.sum(x)), rel=rel, abs=1e-300)
    assert st.sumsq == pytest.approx(float(np.sum(x * x)), rel=2 * rel, abs=1e-300)
    assert st.price == pytest.approx(float(price), rel=rel, abs=1e-300)
    assert float(price) == pytest.approx(disc * float(np.mean(x)), rel=1e-14, abs=1e-300)


# ------------------------------------------------------------------ barrier
KINDS = ("up-and-out", "up-and-in", "down-and-out", "down-and-in")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,B,call,N,M,anti", [
    (100.0, 115.0, True, 20_001, 252, False), (100.0, 85.0, False, 9_999, 101, False), (100.0, 110.0, False, 4_097, 1, False),
    (100.0, 90.0, True, 30_000, 4, False), (100.0, 105.0, True, 20_000, 5, False), (100.0, 95.0, False, 20_000, 6, False),
    (100.0, 120.0, True, 12_345, 7, False), (100.0, 92.0, True, 10_001, 64, True), (100.0, 112.0, False, 7_777, 13, True),
])
def test_barrier_tied_to_reference(kind, S, B, call, N, M, anti):
    level = reference_barrier_level(S, B, kind)
    assert level == B                                                   # away from the spot the level is the contract's
    st = _hip.barrier(S, 100.0, T, R, V, Q, call, level, _hip.BARRIER_KINDS[kind], N, M, SEED, anti)
    price, x = orc.barrier_from_paths(tied_paths(S, N, M, SEED, anti), 100.0, T, R, B, kind, "call" if call else "put", return_payoffs=True)
    assert_tied(st, price, x, MIRROR if anti else EXACT, math.exp(-R * T))


# the reference's column 0 = np.exp(np.log(S)) is above S for 100, below for 80, S itself for 95: a barrier at the spot or one ulp
# either side of it is crossed at t = 0 or not by that value, not by the log-space rule of the C ABI (include/olmc.h)
SPOTS = (100.0, 80.0, 95.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", SPOTS)
@pytest.mark.parametrize("ulps", (-1, 0, 1))
def test_barrier_at_spot_tied_to_reference(kind, S, ulps):
    B = S if ulps == 0 else float(np.nextafter(S, np.inf if ulps > 0 else 0.0))
    N, M = 20_000, 64
    paths = tied_paths(S, N, M, 1)
    for call in (True, False):
        typ = "call" if call else "put"
        price, x = orc.barrier_from_paths(paths, S, T, R, B, kind, typ, return_payoffs=True)
        st = _hip.barrier(S, S, T, R, V, Q, call, reference_barrier_level(S, B, kind), _hip.BARRIER_KINDS[kind], N, M, 1)
        assert_tied(st, price, x, EXACT, math.exp(-R * T))
        # the product layer (BarrierOption here, the fused Greeks below) passes the level that reproduces the reference
        o = ol.BarrierOption(S=S, K=S, T=T, r=R, sigma=V, q=Q, barrier=B, seed=1)
        assert o.price(N, M, kind, typ) == pytest.approx(price, rel=EXACT, abs=1e-300)
    want = orc.barrier_from_paths(paths, S, T, R, B, kind, "call")
    ad = ol.ExoticAdapter(ol.BarrierOption(S=S, K=S, T=T, r=R, sigma=V, q=Q, barrier=B, seed=1), n_paths=N, n_steps=M, barrier_type=kind)
    g = ol.compute_greeks_unified(ad, S, S, T, R, V, "call", Q, include_second_order=False)
    assert g["price"] == pytest.approx(want, rel=EXACT, abs=1e-300)


def test_barrier_at_spot_prices_of_the_issue():
    """20k x 64, seed 1, K = S = B, q = 0: knock-outs the reference prices well above 0 on its own stream, which the log-space rule
    alone would price at exactly 0.  The device's price is the reference's payoff on the device's paths, and within sampling noise
    of the reference's own price."""
    for S, kind, typ, want in ((100.0, "down-and-out", "call", 2.306), (80.0, "up-and-out", "put", 0.863)):
        ref = orc.barrier_price(S, S, T, R, V, S, 0.0, 1, 20_000, 64, kind, typ)
        assert ref == pytest.approx(want, abs=5e-4)
        tied = orc.barrier_from_paths(tied_paths(S, 20_000, 64, 1, q=0.0), S, T, R, S, kind, typ)
        got, se = ol.BarrierOption(S=S, K=S, T=T, r=R, sigma=V, barrier=S, seed=1).price(20_000, 64, kind, typ, return_error=True)
        assert got > 0 and got == pytest.approx(tied, rel=EXACT)
        assert abs(got - ref) <= 3 * math.sqrt(2) * se


def test_price_barrier_helper_at_spot():
    """exotic_options.py:575-590 (n_steps = 252): the reference's helper at a barrier on the spot."""
    for S, kind, typ in ((100.0, "down-and-out", "call"), (80.0, "up-and-out", "put"), (100.0, "down-and-in", "call")):
        got = ol.price_barrier(S, S, T, R, V, S, kind, typ, n_paths=5_001, seed=3)
        want = orc.barrier_from_paths(tied_paths(S, 5_001, 252, 3, q=0.0), S, T, R, S, kind, typ)
        assert got == pytest.approx(want, rel=EXACT, abs=1e-300)


# ------------------------------------------------------------------ lookback
@pytest.mark.parametrize("fixed", (False, True))
@pytest.mark.parametrize("call", (True, False))
@pytest.mark.parametrize("S,N,M,anti", [(100.0, 20_001, 252, False), (80.0, 4_097, 1, False), (95.0, 9_999, 101, False),
                                        (100.0, 30_000, 6, False), (110.0, 20_000, 7, True), (100.0, 8_191, 4, True)])
def test_lookback_tied_to_reference(fixed, call, S, N, M, anti):
    st = _hip.lookback(S, 100.0, T, R, V, Q, call, fixed, N, M, SEED, anti)
    price, x = orc.lookback_from_paths(tied_paths(S, N, M, SEED, anti), 100.0, T, R, "fixed" if fixed else "floating",
                                       "call" if call else "put", return_payoffs=True)
    assert_tied(st, price, x, MIRROR if anti else EXACT, math.exp(-R * T))


# ------------------------------------------------------------------ Asian
@pytest.mark.parametrize("avg", ("arithmetic", "geometric", "fast"))
@pytest.mark.parametrize("call", (True, False))
@pytest.mark.parametrize("S,K,N,M,anti", [(100.0, 100.0, 20_001, 252, False), (100.0, 95.0, 4_097, 1, False),
                                          (90.0, 100.0, 9_999, 101, False), (100.0, 105.0, 30_000, 4, False),
                                          (100.0, 100.0, 20_000, 5, False), (110.0, 100.0, 20_000, 6, False),
                                          (100.0, 100.0, 12_345, 7, True), (100.0, 98.0, 8_191, 64, True)])
def test_asian_tied_to_reference(avg, call, S, K, N, M, anti):
    st = _hip.asian(S, K, T, R, V, Q, call, avg == "geometric", N, M, SEED, anti, fast=avg == "fast")
    price, x = orc.asian_from_paths(tied_paths(S, N, M, SEED, anti), K, T, R, "geometric" if avg == "geometric" else "arithmetic",
                                    "call" if call else "put", return_payoffs=True)
    assert_tied(st, price, x, max(REL if avg != "arithmetic" else EXACT, MIRROR if anti else 0.0), math.exp(-R * T))


# ------------------------------------------------------------------ autocallable
AC = dict(autocall_barrier=1.0, coupon_barrier=0.8, coupon_rate=0.10, ki_barrier=0.6)


@pytest.mark.parametrize("S,N,M,freq,kw,anti", [
    (100.0, 20_001, 252, 21, {}, False),
    (100.0, 9_999, 100, 30, dict(autocall_barrier=1.05, ki_barrier=0.9), False),    # freq does not divide n_steps: 10 trailing steps
    (100.0, 20_000, 50, 60, {}, False),                                            # freq > n_steps: no observation date
    (100.0, 4_097, 1, 2, dict(ki_barrier=0.99), False),
    (100.0, 20_000, 252, 63, dict(autocall_barrier=1.15), False),                  # calls on the last date, which is maturity
    (100.0, 20_000, 13, 13, dict(autocall_barrier=1.02), False),                   # one observation date, on the last step
    (100.0, 12_345, 22, 5, dict(ki_barrier=0.85), False), (100.0, 7_777, 7, 3, {}, False),
    (100.0, 10_001, 126, 21, dict(ki_barrier=0.9), True), (100.0, 5_003, 45, 50, {}, True),
    # ki_barrier = 1.0 with the reference's column 0 above (100), below (80) and at (95) the spot
    (100.0, 20_000, 64, 16, dict(ki_barrier=1.0), False), (80.0, 20_000, 64, 16, dict(ki_barrier=1.0), False),
    (95.0, 20_000, 64, 16, dict(ki_barrier=1.0), False),
])
def test_autocallable_tied_to_reference(S, N, M, freq, kw, anti):
    k = {**AC, **kw}
    rel = MIRROR if anti else EXACT
    price, x = orc.autocallable_from_paths(tied_paths(S, N, M, SEED, anti), S, T, R, freq, return_payoffs=True, **k)
    args = (S, T, R, V, Q, k["autocall_barrier"], k["coupon_barrier"], k["coupon_rate"], k["ki_barrier"], freq, N, M, SEED, anti)
    if freq <= M:
        assert_tied(_hip.autocallable(*args), price, x, rel)
        assert np.any(x != x.max()) and len(np.unique(np.round(x, 12))) > 2   # redemptions on more than one date, or a loss
    else:
        # no observation date: the C ABI refuses it (include/olmc.h); the reference runs every path to maturity, and so does
        # AutocallableOption below (an autocall level no path reaches)
        with pytest.raises(ol.AccelerationError):
            _hip.autocallable(*args)
        assert np.all(x > 0) and len(np.unique(np.round(x, 12))) > 2        # coupon, no coupon, knock-in losses: all at maturity
    o = ol.AutocallableOption(S=S, K=S, T=T, r=R, sigma=V, q=Q, seed=SEED, **k)
    got, se = o.price(N, M, freq, antithetic=anti, return_error=True)
    assert got == pytest.approx(price, rel=rel)
    # payoffs carry their own discount: the standard error is std(x) / sqrt(n) of the same payoffs (cancellation in
    # sumsq/n - mean^2 costs a few digits)
    assert se == pytest.approx(float(np.std(x)) / math.sqrt(len(x)), rel=1e-8)


# ------------------------------------------------------------------ cliquet
@pytest.mark.parametrize("N,M,periods,kw,anti", [
    (20_001, 252, 12, {}, False), (9_999, 100, 12, {}, False),           # 100 % 12 = 4 trailing steps
    (20_000, 250, 12, dict(local_cap=0.08, local_floor=-0.03), False),   # 10 trailing steps
    (20_000, 13, 13, {}, False), (4_097, 1, 1, {}, False),              # n_periods == n_steps
    (20_000, 67, 5, dict(global_cap=0.15, global_floor=-0.1), False), (12_345, 64, 64, {}, True), (8_191, 101, 4, {}, True),
])
def test_cliquet_tied_to_reference(N, M, periods, kw, anti):
    k = {**dict(local_cap=0.05, local_floor=-0.05, global_cap=0.30, global_floor=0.0), **kw}
    st = _hip.cliquet(100.0, T, R, V, Q, k["local_cap"], k["local_floor"], k["global_cap"], k["global_floor"], periods, N, M, SEED, anti)
    price, x = orc.cliquet_from_paths(tied_paths(100.0, N, M, SEED, anti), 100.0, T, R, periods, return_payoffs=True, **k)
    assert_tied(st, price, x, REL, math.exp(-R * T))


# ------------------------------------------------------------------ American (Longstaff-Schwartz)
# Degrees 1-3: the device's normal equations in the standardised regressor and the reference's SVD lstsq on raw powers are the same
# least-squares fit to far below any exercise margin, so no decision flips and the prices agree to 1e-9 (one flip would move them by
# ~1e-5).  Degree 4 is NOT well conditioned on the reference's side: its raw powers of S make a design matrix of condition 1e11-1e13,
# and lstsq's own fit then flips from a few to ~100 exercise decisions per 20k paths against an exact fit (on the reference's own
# paths, 3.5e-4 on the price at most over five seeds) -- so degree 4 is tied at 1e-3, still several times tighter than one standard
# error.  Ill-conditioned and singular regressions keep their own tests in tests/test_gpu_exotics.py.
AMERICAN_TIE = 1e-9
AMERICAN_TIE_DEGREE_4 = 1e-3


@pytest.mark.parametrize("S,K,v,q,call,N,M,deg", [
    (100.0, 100.0, 0.2, 0.0, False, 50_000, 50, 3), (90.0, 100.0, 0.3, 0.0, False, 20_001, 25, 2),
    (100.0, 110.0, 0.25, 0.0, False, 30_000, 52, 1), (95.0, 100.0, 0.15, 0.0, False, 20_000, 13, 3),
    (100.0, 100.0, 0.2, 0.08, True, 20_000, 40, 3), (110.0, 100.0, 0.3, 0.06, True, 10_007, 33, 2),
    (100.0, 90.0, 0.25, 0.05, True, 15_000, 21, 1), (100.0, 100.0, 0.2, 0.0, False, 5_000, 1, 3),
    (100.0, 95.0, 0.25, 0.0, False, 20_000, 13, 4), (100.0, 100.0, 0.4, 0.0, False, 40_000, 6, 4),
])
def test_american_tied_to_reference(S, K, v, q, call, N, M, deg):
    st = _hip.american_lsm(S, K, T, R, v, q, call, N, M, deg, SEED)
    price, x = orc.american_from_paths(tied_paths(S, N, M, SEED, v=v, q=q), K, T, R, "call" if call else "put", deg, return_payoffs=True)
    assert_tied(st, price, x, AMERICAN_TIE_DEGREE_4 if deg == 4 else AMERICAN_TIE)
