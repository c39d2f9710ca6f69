"""Dupire local-volatility paths on the device (include/olmc_local_vol.h) against tests/local_vol_oracle.py and the GBM kernels.

Sizes: N in {100, 257, 4133} paths (less than a workgroup, one thread past a workgroup, 17 workgroups with a ragged last one), n in
{1, 5, 13, 64} steps (a partial Philox block, a block and a bit, three and a bit, sixteen whole blocks).

  1  a flat table gives olmc_gbm_paths' matrix of the flat value: 1e-10 relative, both layouts.  The two differ by rounding only, at
     most n 2^-52 on ln S (about 1e-14), while a wrong normal or date moves a path by 1e-3.
  2  smile tables (n_t, n_x) in {(1, 2), (2, 7), (64, 256), (33, 128)}, distinct nodes with a skew, the (2, 7) one so narrow that paths
     leave it on both sides (asserted from the matrix: at least 1 % of the paths beyond each edge at some date): the oracle's paths on
     normals recovered from the device's own GBM matrix of the same seed equal ollv_paths within 1e-9 relative.  The recovery errs by
     about 1e-15 / (sigma_0 sqrt(dt)), some 4e-14 per normal, 1e-13 on a 64-step path; a wrong cell or weight moves sigma by 1e-4.
  3  every payoff code 0-8, call and put, plain and antithetic: ollv_price's sums equal the payoffs NumPy computes from the rows of
     ollv_paths (for the mirrored leg: the oracle's rows on -z) within 1e-9 relative, at every N x n, on the typical table, the narrow
     one (paths on the flat edges) and the caps' 64 x 256.  No path comes within 1e-9 of a barrier level in
     log space at any date (asserted from the matrices), so none is excluded.
  4  ollv_surface_prices: five cells at steps 2, 4, 5, 13, 64 of 64 (on and off Philox block boundaries) equal the column payoffs, at every N,
     on the typical and the narrow table.
  5  shards [0, 100) + [100, 257) through olmc_combine_stats equal the whole within 1e-12.
  6  under OLMC_TUNE_GRID_CAP = 1 ollv_paths keeps its bits and the sums stay within 1e-12.
  7  flat 0.2, 2^16 paths x 16 steps: the European price is within 3 standard errors of black_scholes.
  8  S = NaN gives a NaN price, and the next call is right.

Every tie prints its worst deviation as a `DEVIATION {json}` line.

The device's own GBM matrix, which 1 compares with and whose normals 2 recovers (an error of its fp64 part would go into them unseen),
is pinned in tests/test_gpu_path_matrices_exact.py to a long-double recursion on the stream's draws.
"""
import contextlib
import json

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import local_vol_oracle as lvo

pytestmark = pytest.mark.gpu

PATHS = (100, 257, 4133)
STEPS = (1, 5, 13, 64)
S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
SIGMA0 = 0.2                                      # the GBM matrix the normals are recovered from
SEED = (0x9E3779B9 << 32) | 20240229              # a non-zero high key word
UP, DOWN = 112.0, 90.0
EUROPEAN = _hip.LV_EUROPEAN


def smile(n_t, n_x, x_lo, x_hi, t_hi):
    """Distinct nodes with a skew and a term structure: 0.22 - 0.25 x + 0.4 x^2 + 0.05 tau / t_hi, all within [0.15, 0.55]."""
    table = lvo.smile_table(n_t, n_x, x_lo, x_hi, t_hi)
    vol = table.vol
    a = vol.astype(np.float32)                                # what the kernels read: every node differs from its neighbours
    assert len(np.unique(vol)) == vol.size and np.all(np.diff(a, axis=1) != 0) and np.all(np.diff(a, axis=0) != 0) and vol.min() > 0.15
    return table


TABLES = {
    "1x2": smile(1, 2, -0.4, 0.3, 1.0),
    "2x7-narrow": smile(2, 7, -0.02, 0.015, 0.6),            # paths leave it on both sides; flat in time beyond 0.6
    "64x256": smile(64, 256, -0.6, 0.5, 1.0),                # the caps: 64 KiB of LDS
    "33x128": smile(33, 128, -0.5, 0.45, 0.8),               # the typical shape
}
FLAT = lvo.Table(np.full((3, 5), 0.25), -0.3, 0.3, 0.5)      # 0.25 is exact in fp32

_normals, _matrices = {}, {}


def deviation(**fields):
    print("DEVIATION " + json.dumps(fields))


def rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def normals(N, n):
    """z[N, n] of the GBM stream for SEED, recovered from the device's own olmc_gbm_paths matrix; computed once per shape."""
    if (N, n) not in _normals:
        _normals[N, n] = lvo.gbm_normals(_hip.gbm_paths(S, T, R, SIGMA0, Q, N, n, SEED, path_major=True), T, R, SIGMA0, Q)
    return _normals[N, n]


def matrices(name, N, n):
    """(the device's ollv_paths matrix, the oracle's matrix on -z) for a table and a shape; computed once."""
    if (name, N, n) not in _matrices:
        table = TABLES[name]
        _matrices[name, N, n] = (_hip.lv_paths(S, T, R, Q, table.args, N, n, SEED, path_major=True), lvo.paths(-normals(N, n), table, S, T, R, Q))
    return _matrices[name, N, n]


@contextlib.contextmanager
def grid_cap(value):
    _hip.tune(_hip.TUNE_GRID_CAP, value)
    try:
        yield
    finally:
        _hip.tune(_hip.TUNE_GRID_CAP, 0)


@pytest.fixture(scope="module", autouse=True)
def device():
    if not _hip.hip_available():
        pytest.fail("no HIP device")


# 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", PATHS)
def test_flat_table_is_the_gbm_matrix(N):
    worst = 0.0
    for n in STEPS:
        for path_major in (True, False):
            want = _hip.gbm_paths(S, T, R, 0.25, Q, N, n, SEED, path_major=path_major)
            got = _hip.lv_paths(S, T, R, Q, FLAT.args, N, n, SEED, path_major=path_major)
            assert got.shape == want.shape
            assert np.array_equal(got[:, 0] if path_major else got[0], np.full(N, S))
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-10, (N, n, path_major)
    deviation(test="flat-vs-gbm", N=N, worst_rel=worst)


# 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLES))
def test_smile_table_paths_equal_the_oracle(name):
    table = TABLES[name]
    worst = 0.0
    for N in PATHS:
        for n in STEPS:
            got, _mirror = matrices(name, N, n)
            want = lvo.paths(normals(N, n), table, S, T, R, Q)
            assert np.array_equal(got[:, 0], np.full(N, S))
            if name == "2x7-narrow":
                x = np.log(got / S)
                assert np.mean((x > table.x_hi).any(axis=1)) >= 0.01 and np.mean((x < table.x_lo).any(axis=1)) >= 0.01, (N, n)
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-9, (name, N, n)
            time_major = _hip.lv_paths(S, T, R, Q, table.args, N, n, SEED, path_major=False)
            assert np.array_equal(time_major.T, got)
    deviation(test="smile-vs-oracle", table=name, worst_rel=worst)


# 3 ----------------------------------------------------------------------------------------------------------------------
PAYOFF_TABLES = ("33x128", "2x7-narrow", "64x256")          # the typical shape, paths on the flat edges, the caps' 64 KiB of LDS


@pytest.mark.parametrize("name", PAYOFF_TABLES)
def test_every_payoff_equals_the_payoff_of_the_matrix_rows(name):
    table = TABLES[name]
    worst = 0.0
    for N in PATHS:
        for n in STEPS:
            plain, mirror = matrices(name, N, n)
            both = np.concatenate([plain, mirror])
            for level in (UP, DOWN):                       # no path of either leg within 1e-9 of a level in log space, at any date
                assert np.min(np.abs(np.log(both / level))) > 1e-9, (N, n, level)
            for code in range(9):
                level = UP if code <= 1 else DOWN if code <= 3 else 0.0
                for is_call in (True, False):
                    for anti in (False, True):
                        x = lvo.payoff(both if anti else plain, code, is_call, K, level)
                        st = _hip.lv_price(S, K, T, R, Q, is_call, table.args, code, level, N, n, SEED, anti)
                        assert st.n == x.size
                        for got, want in ((st.sum, float(np.sum(x))), (st.sumsq, float(np.sum(x * x)))):
                            assert abs(got - want) <= 1e-9 * abs(want), (N, n, code, is_call, anti, got, want)
                            if want:
                                worst = max(worst, abs(got - want) / abs(want))
                        assert st.price == pytest.approx(np.exp(-R * T) * np.mean(x), rel=1e-9, abs=0.0)
    deviation(test="payoffs-vs-rows", table=name, worst_rel=worst)


# 4 ----------------------------------------------------------------------------------------------------------------------
CELL_STEPS = (2, 4, 5, 13, 64)
CELL_STRIKES = (90.0, 95.0, 100.0, 105.0, 110.0)


@pytest.mark.parametrize("name", ("33x128", "2x7-narrow"))
@pytest.mark.parametrize("N", PATHS)
def test_surface_cells_equal_the_column_payoffs(N, name):
    n = 64
    plain, mirror = matrices(name, N, n)
    both = np.concatenate([plain, mirror])
    order = (3, 0, 4, 2, 1)                        # the caller's order is not the steps' order
    strikes, steps = [CELL_STRIKES[i] for i in order], [CELL_STEPS[i] for i in order]
    worst = 0.0
    for is_call in (True, False):
        for anti in (False, True):
            rows = both if anti else plain
            sts = _hip.lv_surface_prices(S, T, R, Q, is_call, TABLES[name].args, strikes, steps, N, n, SEED, anti)
            assert len(sts) == 5
            for st, strike, m in zip(sts, strikes, steps):
                x = np.maximum((1.0 if is_call else -1.0) * (rows[:, m] - strike), 0.0)
                assert st.n == x.size
                for got, want in ((st.sum, float(np.sum(x))), (st.sumsq, float(np.sum(x * x)))):
                    assert abs(got - want) <= 1e-9 * abs(want), (is_call, anti, strike, m, got, want)
                    if want:
                        worst = max(worst, abs(got - want) / abs(want))
                assert st.price == pytest.approx(np.exp(-R * T * m / n) * np.mean(x), rel=1e-9, abs=0.0)
    deviation(test="surface-vs-columns", table=name, N=N, worst_rel=worst)


# 5 ----------------------------------------------------------------------------------------------------------------------
def combined(parts, t):
    return _hip.combine_stats([(p.sum, p.sumsq, p.n) for p in parts], R, t)


def same(a, b, tol=1e-12):
    return a.n == b.n and all(abs(getattr(a, f) - getattr(b, f)) <= tol * abs(getattr(b, f)) for f in ("sum", "sumsq", "price", "std_error"))


@pytest.mark.parametrize("n", (5, 64))
def test_shards_add_up(n):
    table = TABLES["33x128"].args
    for anti in (False, True):
        for code, level in ((0, UP), (3, DOWN), (5, 0.0), (6, 0.0), (7, 0.0), (EUROPEAN, 0.0)):
            whole = _hip.lv_price(S, K, T, R, Q, True, table, code, level, 257, n, SEED, anti)
            parts = [_hip.lv_price(S, K, T, R, Q, True, table, code, level, cnt, n, SEED, anti, path_offset=off) for off, cnt in ((0, 100), (100, 157))]
            assert same(combined(parts, T), whole), (code, anti)
        steps = [min(m, n) for m in (2, 5, 64)]
        whole = _hip.lv_surface_prices(S, T, R, Q, False, table, [95.0, 100.0, 105.0], steps, 257, n, SEED, anti)
        parts = [_hip.lv_surface_prices(S, T, R, Q, False, table, [95.0, 100.0, 105.0], steps, cnt, n, SEED, anti, path_offset=off)
                 for off, cnt in ((0, 100), (100, 157))]
        for j, m in enumerate(steps):
            assert same(combined([p[j] for p in parts], T * m / n), whole[j]), (j, anti)


# 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("33x128", "64x256"))
def test_one_workgroup_walks_every_path_to_the_same_result(name):
    table, N, n = TABLES[name].args, 4133, 13
    free_matrix = _hip.lv_paths(S, T, R, Q, table, N, n, SEED, path_major=True)
    free = {(code, anti): _hip.lv_price(S, K, T, R, Q, False, table, code, level, N, n, SEED, anti)
            for code, level in ((1, UP), (4, 0.0), (6, 0.0), (EUROPEAN, 0.0)) for anti in (False, True)}
    free_cells = _hip.lv_surface_prices(S, T, R, Q, True, table, [95.0, 105.0], [5, 13], N, n, SEED, True)
    with grid_cap(1):
        assert np.array_equal(_hip.lv_paths(S, T, R, Q, table, N, n, SEED, path_major=True), free_matrix)
        assert np.array_equal(_hip.lv_paths(S, T, R, Q, table, N, n, SEED, path_major=False).T, free_matrix)
        for (code, anti), want in free.items():
            level = UP if code == 1 else 0.0
            assert same(_hip.lv_price(S, K, T, R, Q, False, table, code, level, N, n, SEED, anti), want), (code, anti)
        for got, want in zip(_hip.lv_surface_prices(S, T, R, Q, True, table, [95.0, 105.0], [5, 13], N, n, SEED, True), free_cells):
            assert same(got, want)


# 7 ----------------------------------------------------------------------------------------------------------------------
def test_flat_twenty_percent_prices_black_scholes():
    table = (np.full((1, 2), 0.2), -1.0, 1.0, 1.0)
    for is_call in (True, False):
        st = _hip.lv_price(S, K, T, R, Q, is_call, table, EUROPEAN, 0.0, 1 << 16, 16, SEED, False)
        bs = ol.black_scholes(S, K, T, R, 0.2, "call" if is_call else "put", Q)
        deviation(test="black-scholes", is_call=is_call, price=st.price, bs=bs, std_errors=abs(st.price - bs) / st.std_error)
        assert abs(st.price - bs) <= 3.0 * st.std_error
    model = ol.DupireLocalVol(n_paths=1 << 16, n_steps=16, seed=SEED)          # uncalibrated: the same flat 0.2, through the Python class
    assert model.price(S, K, T, R, 0.9, "call", Q) == _hip.lv_price(S, K, T, R, Q, True, table, EUROPEAN, 0.0, 1 << 16, 16, SEED, False).price


# 8 ----------------------------------------------------------------------------------------------------------------------
def test_nan_spot_gives_nan_and_the_next_call_is_right():
    table = TABLES["33x128"].args
    before = _hip.lv_price(S, K, T, R, Q, True, table, EUROPEAN, 0.0, 257, 13, SEED, True)
    bad = _hip.lv_price(float("nan"), K, T, R, Q, True, table, EUROPEAN, 0.0, 257, 13, SEED, True)
    assert np.isnan(bad.price) and np.isnan(bad.std_error) and np.isnan(bad.sum) and bad.n == 514
    assert all(np.isnan(c.price) for c in _hip.lv_surface_prices(float("nan"), T, R, Q, True, table, [100.0], [13], 257, 13, SEED))
    assert np.isnan(_hip.lv_paths(float("nan"), T, R, Q, table, 100, 5, SEED, path_major=True)[:, 1:]).all()
    after = _hip.lv_price(S, K, T, R, Q, True, table, EUROPEAN, 0.0, 257, 13, SEED, True)
    assert (after.sum, after.sumsq, after.n, after.price) == (before.sum, before.sumsq, before.n, before.price) and np.isfinite(after.price)


# the calibrated model end to end: the reference's sample surface through the Python class ---------------------------------------
def test_calibrated_model_prices_through_the_python_class():
    strikes, expiries, iv = ol.create_sample_iv_surface()
    model = ol.DupireLocalVol(r=R, q=0.0, n_paths=4133, n_steps=13, seed=7)
    model.calibrate(strikes, expiries, iv, 100.0)
    table = model.local_vol_table(S, T)
    paths = model.simulate_paths(S, T, R, 0.0, 4133, 13, 7)
    assert paths.shape == (4133, 14) and np.array_equal(paths, _hip.lv_paths(S, T, R, 0.0, table, 4133, 13, 7, path_major=True))
    price, err = model.price_monte_carlo(S, K, T, R, 0.0, "call", return_error=True)
    x = np.maximum(paths[:, -1] - K, 0.0)
    assert price == pytest.approx(np.exp(-R * T) * x.mean(), rel=1e-9) and err == pytest.approx(np.exp(-R * T) * x.std() / np.sqrt(4133), rel=1e-9)
    assert model.price(S, K, T, R, 0.5, "call") == price
    assert model.price_asian(S, K, T, R) == pytest.approx(np.exp(-R * T) * np.maximum(paths[:, 1:].mean(axis=1) - K, 0.0).mean(), rel=1e-9)
    assert model.price_lookback(S, K, T, R, option_type="put") == pytest.approx(np.exp(-R * T) * (paths.max(axis=1) - paths[:, -1]).mean(), rel=1e-9)
    alive = paths.max(axis=1) < 125.0
    assert model.price_barrier(S, K, T, R, 125.0) == pytest.approx(np.exp(-R * T) * np.where(alive, x, 0.0).mean(), rel=1e-9)
    surface = model.price_surface(S, [95.0, 105.0], [5 / 13, 1.0], R)
    assert surface.shape == (2, 2)
    assert surface[1, 1] == pytest.approx(np.exp(-R * T) * np.maximum(paths[:, -1] - 105.0, 0.0).mean(), rel=1e-9)
    assert surface[0, 0] == pytest.approx(np.exp(-R * T * 5 / 13) * np.maximum(paths[:, 5] - 95.0, 0.0).mean(), rel=1e-9)
