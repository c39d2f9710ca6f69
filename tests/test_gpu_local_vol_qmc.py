"""Dupire local-volatility paths on scrambled-Sobol points (include/olmc_local_vol_qmc.h) against tests/local_vol_oracle.py on SciPy's points.

The oracle is a composition of what the suite already pins (tests/test_local_vol_qmc_cpu.py checks it on a flat table): z = SciPy's
Sobol(d = n, scramble=True, seed) normals (sobol_reference.normal_chunks), then lvo.paths(z, ...) for the sequential construction and
lvo.paths(np.diff(bridge_walk(z), axis=1), ...) for the bridge; the mirror leg is the same on -z.

Sizes: N in {1, 65, 257, 4133} points (one lane; a block of 64 and a lane; four waves and a lane; 17 workgroups with a ragged tail), n in
{1, 2, 13, 64, 65, 252, 1024} steps (a single node; a batch of 4 cut short; 13; one whole fold of 64 dimensions; a fold plus one; 252;
the bridge's cap) and n = 1025 for the sequential construction alone.  CASES lets each n meet each table once and each N once (a Latin
square), not the full product.  Tables: tests/test_gpu_local_vol.py's.

  1  olvq_paths equals the oracle's matrix within 1e-10 relative (the project's QMC bar, tests/test_gpu_heston_qmc.py), both
     constructions, both layouts; column 0 is S.  On the narrow table at least 1 % of the paths leave it on each side (N >= 65).
  2  every payoff code 0-8, call and put, plain and antithetic, both constructions: olvq_price's sum and sumsq equal the payoffs
     lvo.payoff computes from the oracle's rows (and the mirror's) within 1e-10 relative; n is the sample count.  No path of either leg
     comes within 1e-9 of a barrier level in log space (tests/test_local_vol_qmc_cpu.py asserts it for these CASES): none is excluded.
  3  olvq_surface_prices: five cells at steps 2, 4, 5, 13, 64 of 64 in a shuffled order equal the column payoffs, discounted over the
     cell's own time.
  4  shards [0, 100) + [100, 257) (the second starts inside a block of 64) combine to the whole within 1e-12, price and surface.
  5  under OLMC_TUNE_GRID_CAP = 1 the matrix keeps its bits and the sums stay within 1e-12: one workgroup strides over every block and
     reuses its slabs.
  6  flat 0.2, 2^14 points x 16 steps, bridge: the European price is within 1e-3 of Black-Scholes, and within twice the gap the CPU
     oracle has on the same points.
  7  S = NaN gives NaN, and the next call gives the earlier bits; with profiling on, one call of each entry point counts as one launch.
  8  a calibrated sample surface through model.qmc(): simulate_paths is _hip.lvq_paths on local_vol_table, the pricing methods equal
     NumPy on that matrix within 1e-9, price() is price_monte_carlo.
  9  2^12 x 64 on "33x128": the standard deviation over 16 scrambles of codes 6 and 8 is at least 10 x smaller than over 16 Philox seeds
     (the CPU prototype: 26 x and 83 x; a standard deviation from 16 samples is good to about +-36 % at 95 %).

Every tie prints its worst deviation as a `DEVIATION {json}` line.
"""
import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.monte_carlo import sobol_tables
from tests import local_vol_oracle as lvo
from tests.sobol_reference import bridge_walk, normal_chunks
from tests.test_gpu_local_vol import DOWN, EUROPEAN, K, Q, R, S, T, TABLES, UP, combined, deviation, grid_cap, rel, same

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

POINTS = (1, 65, 257, 4133)
STEPS = (1, 2, 13, 64, 65, 252, 1024)
SEQUENTIAL_ONLY_STEPS = 1025                      # beyond the bridge's cap
SEED = 20240229
NAMES = list(TABLES)
# (table, N, n): step count i meets table j at N = POINTS[(i + j) % 4]
CASES = [(name, POINTS[(i + j) % 4], n) for i, n in enumerate(STEPS + (SEQUENTIAL_ONLY_STEPS,)) for j, name in enumerate(NAMES)]

_normals, _oracle = {}, {}


def constructions(n):
    return (False, True) if n <= _hip.QMC_BRIDGE_MAX_STEPS else (False,)


def normals(N, n, seed=SEED):
    """z[N, n] of SciPy's scrambled Sobol points 0 .. N - 1; computed once per shape."""
    if (N, n, seed) not in _normals:
        _normals[N, n, seed] = np.concatenate(list(normal_chunks(n, N, seed, 4096)))
    return _normals[N, n, seed]


def increments(z, bridge):
    return np.diff(bridge_walk(z), axis=1) if bridge else z


def oracle(name, N, n, bridge):
    """(the oracle's matrix, its matrix on the mirrored point -z) for a table, a shape and a construction; computed once."""
    if (name, N, n, bridge) not in _oracle:
        dw = increments(normals(N, n), bridge)
        _oracle[name, N, n, bridge] = (lvo.paths(dw, TABLES[name], S, T, R, Q), lvo.paths(-dw, TABLES[name], S, T, R, Q))
    return _oracle[name, N, n, bridge]


def level_of(code):
    return UP if code <= 1 else DOWN if code <= 3 else 0.0


@pytest.fixture(scope="module", autouse=True)
def device():
    if not _hip.hip_available():
        pytest.fail("no HIP device")


# 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_paths_equal_the_oracle(name):
    table = TABLES[name]
    worst = 0.0
    for _name, N, n in [c for c in CASES if c[0] == name]:
        sv, shift = sobol_tables(n, SEED, N)
        for bridge in constructions(n):
            want, _mirror = oracle(name, N, n, bridge)
            got = _hip.lvq_paths(S, T, R, Q, table.args, N, sv, shift, bridge, path_major=True)
            assert got.shape == want.shape == (N, n + 1) and np.array_equal(got[:, 0], np.full(N, S))
            if name == "2x7-narrow" and N >= 65:
                x = np.log(got / S)
                assert np.mean((x > table.x_hi).any(axis=1)) >= 0.01 and np.mean((x < table.x_lo).any(axis=1)) >= 0.01, (N, n, bridge)
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-10, (name, N, n, bridge, rel(got, want))
            time_major = _hip.lvq_paths(S, T, R, Q, table.args, N, sv, shift, bridge, path_major=False)
            assert np.array_equal(time_major.T, got), (name, N, n, bridge)
    deviation(test="qmc-paths-vs-oracle", table=name, worst_rel=worst)


# 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_payoff_equals_the_payoff_of_the_oracle_s_rows(name):
    table = TABLES[name]
    worst = 0.0
    for _name, N, n in [c for c in CASES if c[0] == name]:
        sv, shift = sobol_tables(n, SEED, N)
        for bridge in constructions(n):
            plain, mirror = oracle(name, N, n, bridge)
            both = np.concatenate([plain, mirror])
            for code in range(9):
                for is_call in (True, False):
                    for anti in (False, True):
                        x = lvo.payoff(both if anti else plain, code, is_call, K, level_of(code))
                        st = _hip.lvq_price(S, K, T, R, Q, is_call, table.args, code, level_of(code), N, sv, shift, bridge, anti)
                        assert st.n == x.size
                        for got, want in ((st.sum, float(np.sum(x))), (st.sumsq, float(np.sum(x * x)))):
                            assert abs(got - want) <= 1e-10 * abs(want), (N, n, bridge, code, is_call, anti, got, want)
                            if want:
                                worst = max(worst, abs(got - want) / abs(want))
                        assert st.price == pytest.approx(np.exp(-R * T) * np.mean(x), rel=1e-10, abs=0.0)
    deviation(test="qmc-payoffs-vs-rows", table=name, worst_rel=worst)


# 3 ----------------------------------------------------------------------------------------------------------------------
CELL_STEPS = (2, 4, 5, 13, 64)
CELL_STRIKES = (90.0, 95.0, 100.0, 105.0, 110.0)


@pytest.mark.parametrize("name", ("33x128", "2x7-narrow"))
@pytest.mark.parametrize("N", POINTS)
def test_surface_cells_equal_the_column_payoffs(N, name):
    n = 64
    sv, shift = sobol_tables(n, SEED, N)
    order = (3, 0, 4, 2, 1)                        # the caller's order is not the steps' order
    strikes, steps = [CELL_STRIKES[i] for i in order], [CELL_STEPS[i] for i in order]
    worst = 0.0
    for bridge in (False, True):
        plain, mirror = oracle(name, N, n, bridge)
        both = np.concatenate([plain, mirror])
        for is_call in (True, False):
            for anti in (False, True):
                rows = both if anti else plain
                sts = _hip.lvq_surface_prices(S, T, R, Q, is_call, TABLES[name].args, strikes, steps, N, sv, shift, bridge, anti)
                assert len(sts) == 5
                for st, strike, m in zip(sts, strikes, steps):
                    x = np.maximum((1.0 if is_call else -1.0) * (rows[:, m] - strike), 0.0)
                    assert st.n == x.size
                    for got, want in ((st.sum, float(np.sum(x))), (st.sumsq, float(np.sum(x * x)))):
                        assert abs(got - want) <= 1e-10 * abs(want), (bridge, is_call, anti, strike, m, got, want)
                        if want:
                            worst = max(worst, abs(got - want) / abs(want))
                    assert st.price == pytest.approx(np.exp(-R * T * m / n) * np.mean(x), rel=1e-10, abs=0.0)
    deviation(test="qmc-surface-vs-columns", table=name, N=N, worst_rel=worst)


# 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (13, 64))
def test_shards_add_up(n):
    table = TABLES["33x128"].args
    sv, shift = sobol_tables(n, SEED, 257)
    for bridge in (False, True):
        for anti in (False, True):
            for code in (0, 3, 5, 6, 7, EUROPEAN):
                whole = _hip.lvq_price(S, K, T, R, Q, True, table, code, level_of(code), 257, sv, shift, bridge, anti)
                parts = [_hip.lvq_price(S, K, T, R, Q, True, table, code, level_of(code), cnt, sv, shift, bridge, anti, point_offset=off)
                         for off, cnt in ((0, 100), (100, 157))]
                assert same(combined(parts, T), whole), (bridge, code, anti)
            steps = [min(m, n) for m in (2, 5, 64)]
            whole = _hip.lvq_surface_prices(S, T, R, Q, False, table, [95.0, 100.0, 105.0], steps, 257, sv, shift, bridge, anti)
            parts = [_hip.lvq_surface_prices(S, T, R, Q, False, table, [95.0, 100.0, 105.0], steps, cnt, sv, shift, bridge, anti, point_offset=off)
                     for off, cnt in ((0, 100), (100, 157))]
            for j, m in enumerate(steps):
                assert same(combined([p[j] for p in parts], T * m / n), whole[j]), (bridge, j, anti)


# 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("33x128", "64x256"))
def test_one_workgroup_walks_every_block_to_the_same_result(name):
    table, N, n = TABLES[name].args, 4133, 13
    sv, shift = sobol_tables(n, SEED, N)
    for bridge in (False, True):
        free_matrix = _hip.lvq_paths(S, T, R, Q, table, N, sv, shift, bridge, path_major=True)
        free = {(code, anti): _hip.lvq_price(S, K, T, R, Q, False, table, code, level_of(code), N, sv, shift, bridge, anti)
                for code in (1, 4, 6, EUROPEAN) for anti in (False, True)}
        free_cells = _hip.lvq_surface_prices(S, T, R, Q, True, table, [95.0, 105.0], [5, 13], N, sv, shift, bridge, True)
        with grid_cap(1):
            assert np.array_equal(_hip.lvq_paths(S, T, R, Q, table, N, sv, shift, bridge, path_major=True), free_matrix)
            assert np.array_equal(_hip.lvq_paths(S, T, R, Q, table, N, sv, shift, bridge, path_major=False).T, free_matrix)
            for (code, anti), want in free.items():
                assert same(_hip.lvq_price(S, K, T, R, Q, False, table, code, level_of(code), N, sv, shift, bridge, anti), want), (bridge, code, anti)
            for got, want in zip(_hip.lvq_surface_prices(S, T, R, Q, True, table, [95.0, 105.0], [5, 13], N, sv, shift, bridge, True), free_cells):
                assert same(got, want)


# 6 ----------------------------------------------------------------------------------------------------------------------
BS_POINTS, BS_STEPS = 1 << 14, 16
BS_TABLE = lvo.Table(np.full((1, 2), 0.2), -1.0, 1.0, 1.0)


def black_scholes_gap_of_the_oracle(is_call):
    """|the oracle's price on the same points - Black-Scholes|: what the bridge leaves at 2^14 points (also asserted <= 1e-3 on the CPU)."""
    spot = lvo.paths(increments(normals(BS_POINTS, BS_STEPS), True), BS_TABLE, S, T, R, Q)
    price = np.exp(-R * T) * np.mean(lvo.payoff(spot, EUROPEAN, is_call, K))
    return abs(price - ol.black_scholes(S, K, T, R, 0.2, "call" if is_call else "put", Q))


def test_flat_twenty_percent_prices_black_scholes():
    sv, shift = sobol_tables(BS_STEPS, SEED, BS_POINTS)
    for is_call in (True, False):
        st = _hip.lvq_price(S, K, T, R, Q, is_call, BS_TABLE.args, EUROPEAN, 0.0, BS_POINTS, sv, shift, True, False)
        bs = ol.black_scholes(S, K, T, R, 0.2, "call" if is_call else "put", Q)
        gap = black_scholes_gap_of_the_oracle(is_call)
        deviation(test="qmc-black-scholes", is_call=is_call, price=st.price, bs=bs, gap=abs(st.price - bs), oracle_gap=gap)
        assert abs(st.price - bs) <= 1e-3 and abs(st.price - bs) <= 2.0 * gap


# 7 ----------------------------------------------------------------------------------------------------------------------
def test_nan_spot_gives_nan_and_the_next_call_is_right():
    table = TABLES["33x128"].args
    sv, shift = sobol_tables(13, SEED, 257)
    nan = float("nan")
    before = _hip.lvq_price(S, K, T, R, Q, True, table, EUROPEAN, 0.0, 257, sv, shift, True, True)
    bad = _hip.lvq_price(nan, K, T, R, Q, True, table, EUROPEAN, 0.0, 257, sv, shift, True, True)
    assert np.isnan(bad.price) and np.isnan(bad.std_error) and np.isnan(bad.sum) and bad.n == 514
    assert all(np.isnan(c.price) for c in _hip.lvq_surface_prices(nan, T, R, Q, True, table, [100.0], [13], 257, sv, shift))
    assert np.isnan(_hip.lvq_paths(nan, T, R, Q, table, 100, sv, shift, True, path_major=True)[:, 1:]).all()
    after = _hip.lvq_price(S, K, T, R, Q, True, table, EUROPEAN, 0.0, 257, sv, shift, True, True)
    assert (after.sum, after.sumsq, after.n, after.price) == (before.sum, before.sumsq, before.n, before.price) and np.isfinite(after.price)


def test_with_profiling_on_one_call_counts_as_one_launch():
    table = TABLES["33x128"].args
    sv, shift = sobol_tables(13, SEED, 257)
    _hip.profile_enable(True)
    try:
        for bridge in (False, True):
            for call in (lambda: _hip.lvq_price(S, K, T, R, Q, True, table, 6, 0.0, 257, sv, shift, bridge, True),
                         lambda: _hip.lvq_paths(S, T, R, Q, table, 257, sv, shift, bridge),
                         lambda: _hip.lvq_surface_prices(S, T, R, Q, True, table, [100.0], [13], 257, sv, shift, bridge)):
                _hip.profile_reset()
                call()
                launches, ms = _hip.kernel_time()
                assert launches == 1 and ms > 0.0
    finally:
        _hip.profile_enable(False)


# 8 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("construction", ("bridge", "sequential"))
def test_calibrated_model_prices_through_the_python_class(construction):
    strikes, expiries, iv = ol.create_sample_iv_surface()
    base = ol.DupireLocalVol(r=R, q=0.0, n_paths=4133, n_steps=13, seed=7)
    base.calibrate(strikes, expiries, iv, 100.0)
    model = base.qmc(construction)
    table = model.local_vol_table(S, T)
    sv, shift = sobol_tables(13, 7, 4133)
    paths = model.simulate_paths(S, T, R, 0.0, 4133, 13, 7)
    assert paths.shape == (4133, 14)
    assert np.array_equal(paths, _hip.lvq_paths(S, T, R, 0.0, table, 4133, sv, shift, construction == "bridge", path_major=True))
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


# 9 ----------------------------------------------------------------------------------------------------------------------
def test_sixteen_scrambles_scatter_ten_times_less_than_sixteen_philox_seeds():
    table, N, n = TABLES["33x128"].args, 1 << 12, 64
    for code in (6, EUROPEAN):
        sobol = [_hip.lvq_price(S, K, T, R, Q, True, table, code, 0.0, N, *sobol_tables(n, s, N), True, False).price for s in range(16)]
        philox = [_hip.lv_price(S, K, T, R, Q, True, table, code, 0.0, N, n, 1000 + s, False).price for s in range(16)]
        ratio = float(np.std(philox, ddof=1) / np.std(sobol, ddof=1))
        deviation(test="qmc-scatter", code=code, N=N, n=n, philox_std=float(np.std(philox, ddof=1)), sobol_std=float(np.std(sobol, ddof=1)), ratio=ratio)
        assert ratio >= 10.0, (code, ratio)
