"""SABR paths on the device (include/olmc_sabr.h) against tests/sabr_oracle.py, NumPy payoffs of the device's own rows, closed forms and
Hagan's expansion.

Sizes: N in {100, 257, 4133} paths (less than a workgroup, one thread past a workgroup, 17 workgroups with a ragged last one), n in
{1, 5, 13, 64} steps (half a Philox block, two and a half, six and a half, 32 whole).  Models (alpha, beta, rho, nu): one per kernel
kind (beta = 1, 0.5, general 0.7) and two that absorb (beta = 0 and beta = 0.5, volatile enough to reach 0).

  1  olsb_paths equals the long-double recursion on the device's own draws (the Philox words of the CPU oracle through the instrumented
     build's Box-Muller tap) within test_gpu_path_matrices_exact.py's TIE (rel 1e-10, abs 1e-12), the forward relative to
     max(|F|, 1e-2 F_0): both layouts, plain and mirror; the (path, date) zeros are the same set on both sides.  Asserted from the oracle,
     none set aside: no pre-clamp G within 1e-7 of 0; each absorbing model absorbs at least 2 % of 4133 paths at 64 steps.
  2  every payoff code 0-8, call and put, plain and antithetic, every model, every N x n: olsb_price's sums equal the payoffs NumPy
     computes from olsb_paths' rows within 1e-9 relative (test_gpu_local_vol.py's bar).  Barriers 112 and 90; no live state within 1e-9
     of a level in log space, asserted.
  3  olsb_surface_prices: cells at steps 2, 4, 5, 13, 64 of 64 in scrambled order with a repeat equal the column payoffs within 1e-9; a
     cell's words do not depend on its neighbours.
  4  shards [0, 100) + [100, 257) combine to the whole within 1e-12; 63 paths at offset 2^32 + 5 equal the oracle's payoffs there (the
     bar is what TIE on every state allows a sum: 2e-10 of the paths' largest states, added up); OLMC_TUNE_GRID_CAP = 1 keeps
     olsb_paths' bits and the sums within 1e-12.
  5  closed forms at 2^16 x 16 within 3 standard errors: nu = 0, beta = 1 against Black-76 at alpha; nu = 0, beta = 0, alpha = 20 against
     Bachelier (absorption has probability about 6e-7: a bias below 1e-4).
  6  Hagan at 2^16 x 64, (0.2, 1, -0.3, 0.4) and `half`, K in {80, 100, 120}: |device - SABRModel.price| <= 3 se + 0.021, the 0.021
     being the largest gap between a NumPy prototype of the scheme at 2^20 paths and Hagan's price over these cells.
  7  beta = 0.5 and np.nextafter(0.5, 1) run two different kernels (the dispatch is by exact equality); their matrices agree within TIE.
  8  F = NaN gives NaN and the next call is right; SABRMCAdapter through compute_greeks_unified gives finite first-order Greeks whose
     delta is within 3 se_FD of greeks_sabr's at the mild model, se_FD from a 16-seed scatter at 2^14 x 16.

Every tie prints a `DEVIATION {json}` line before it asserts (pytest -s).  Worst values measured on an MI355X:

  1  forward 0.0069 of TIE (`half-absorbing`; 0.00092 `normal-absorbing`, under 6e-5 for the three that do not absorb), volatility 2.5e-5
     of TIE; 44,516 + 24,806 + 1 zeros at the same states on both sides; absorbed paths 594 / 614 (`normal-absorbing`) and 368 / 384
     (`half-absorbing`), plain / mirror; closest pre-clamp G 3.5e-4.
  2  6.1e-15 relative; the closest approach to a level 6.6e-8 in log space.
  3  7.2e-14 relative (`lognormal`: the read-out forms exp(ln F + x) where the matrix holds F exp(x)); 3.6e-16 for beta < 1.
  4  the shard beyond 2^32: 8.2e-7 of the slack.
  5  Black-76 0.28 and 0.83, Bachelier 0.08 and 0.67 standard errors (call, put).
  6  gaps 0.011 .. 0.028 against bars of 0.099 .. 0.26.
  7  0.0065 of TIE; the two kernels' sums do differ in their last bits.
  8  delta 0.5961 against Hagan's 0.5985, se_FD 0.00086: 2.8 se_FD.
"""
import contextlib
import json
import math

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.greeks import fd_steps
from tests import sabr_oracle as so
from tests.gpu_support import device_fixture

pytestmark = pytest.mark.gpu

_device = device_fixture(after=lambda: _hip.tune(_hip.TUNE_GRID_CAP, 0))

TIE = dict(rel=1e-10, abs=1e-12)
F0, T, R, K = so.F0, so.T, so.R, 100.0
SEED, PATHS, STEPS, MODELS = so.SEED, so.PATHS, so.STEPS, so.MODELS
UP, DOWN = so.UP, so.DOWN
EUROPEAN = _hip.SABR_EUROPEAN
LONG = so.LONG

_draws, _oracle, _device_rows = {}, {}, {}


def TAP(xa, xb):
    from tools.probe import binding as probe

    return probe.box_muller_probe(xa, xb)


def deviation(**fields):
    print("DEVIATION " + json.dumps(fields))


def draws(N, n, offset=0):
    if (N, n, offset) not in _draws:
        _draws[N, n, offset] = so.draws(SEED, offset, N, n, TAP)
    return _draws[N, n, offset]


def oracle(name, N, n, mirror, offset=0):
    """(forward, vol, closest G) of the long-double recursion on the device's draws; computed once."""
    key = (name, N, n, mirror, offset)
    if key not in _oracle:
        _oracle[key] = so.paths(F0, T, MODELS[name], n, *draws(N, n, offset), mirror=mirror)
    return _oracle[key]


def device_rows(name, N, n, mirror):
    """olsb_paths' (forward, vol), path-major; computed once and left unchanged."""
    key = (name, N, n, mirror)
    if key not in _device_rows:
        _device_rows[key] = _hip.sabr_paths(F0, T, MODELS[name], N, n, SEED, mirror=mirror, path_major=True)
    return _device_rows[key]


def tie_units(got, want, floor=0.0):
    """max |got - want| in units of TIE relative to max(|want|, floor): the tie holds where this is <= 1."""
    diff = np.abs((got.astype(LONG) - want).astype(np.float64))
    return float(np.max(diff / np.maximum(TIE["rel"] * np.maximum(np.abs(want.astype(np.float64)), floor), TIE["abs"])))


def words(st):
    return (st.sum, st.sumsq, st.n, st.price, st.std_error)


def same(a, b, tol=1e-12):
    return a.n == b.n and all(abs(getattr(a, f) - getattr(b, f)) <= tol * abs(getattr(b, f)) for f in ("sum", "sumsq", "price", "std_error"))


@contextlib.contextmanager
def grid_cap(value):
    _hip.tune(_hip.TUNE_GRID_CAP, value)
    try:
        yield
    finally:
        _hip.tune(_hip.TUNE_GRID_CAP, 0)


# 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_paths_equal_the_long_double_recursion_on_the_devices_draws(name):
    model = MODELS[name]
    worst = dict(forward=0.0, vol=0.0, closest_g=math.inf, zeros=0)
    for N in PATHS:
        for n in STEPS:
            for mirror in (False, True):
                label = (name, N, n, mirror)
                forward, vol = device_rows(name, N, n, mirror)
                f_tm, v_tm = _hip.sabr_paths(F0, T, model, N, n, SEED, mirror=mirror, path_major=False)
                assert forward.shape == vol.shape == (N, n + 1) and np.array_equal(f_tm.T, forward) and np.array_equal(v_tm.T, vol), label
                assert np.all(forward[:, 0] == F0) and np.all(vol[:, 0] == model[0]), label
                want_f, want_v, closest = oracle(name, N, n, mirror)
                units_f, units_v = tie_units(forward, want_f, 1e-2 * F0), tie_units(vol, want_v)
                zeros_got, zeros_want = forward == 0.0, want_f == 0
                worst.update(forward=max(worst["forward"], units_f), vol=max(worst["vol"], units_v), closest_g=min(worst["closest_g"], closest),
                             zeros=worst["zeros"] + int(zeros_want.sum()))
                assert closest > 1e-7, label                                                 # the clamp's decision is not a matter of rounding
                assert np.array_equal(zeros_got, zeros_want), label
                assert units_f <= 1.0 and units_v <= 1.0, (label, units_f, units_v)
                assert np.all(forward >= 0.0) and np.all(vol > 0.0), label
                if name in so.ABSORBING and (N, n) == (4133, 64):
                    absorbed = int(np.sum(want_f[:, -1] == 0))
                    deviation(test="absorbed", model=name, mirror=mirror, paths=absorbed)
                    assert absorbed >= 0.02 * N, label
                    dead = forward[forward[:, -1] == 0.0]
                    assert all(np.all(row[np.argmax(row == 0.0):] == 0.0) for row in dead)   # absorbed: 0 at every later date
    deviation(test="paths-vs-oracle", model=name, forward_tie_units=worst["forward"], vol_tie_units=worst["vol"],
              closest_g=None if math.isinf(worst["closest_g"]) else worst["closest_g"], zeros=worst["zeros"])
    if name == "lognormal":
        a, b = ol.SABRModel(*model).simulate_paths(F0, T, 257, 13, SEED, mirror=True)       # the public method is this matrix
        assert np.array_equal(a, device_rows(name, 257, 13, True)[0]) and np.array_equal(b, device_rows(name, 257, 13, True)[1])


# 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_every_payoff_equals_the_payoff_of_the_matrix_rows(name):
    model = MODELS[name]
    worst, clearance = 0.0, math.inf
    for N in PATHS:
        for n in STEPS:
            plain, mirror = device_rows(name, N, n, False)[0], device_rows(name, N, n, True)[0]
            both = np.concatenate([plain, mirror])
            clearance = min(clearance, so.level_clearance(both))
            assert so.level_clearance(both) > 1e-9, (name, N, n)
            for code in range(9):
                level = so.level_of(code)
                for is_call in (True, False):
                    for anti in (False, True):
                        x = so.payoffs(both if anti else plain, code, is_call, K, level)
                        st = _hip.sabr_price(F0, K, T, R, is_call, model, code, level, N, n, SEED, anti)
                        assert st.n == x.size
                        for got, want in ((st.sum, float(np.sum(x))), (st.sumsq, float(np.sum(x * x)))):
                            assert abs(got - want) <= 1e-9 * abs(want), (name, N, n, code, is_call, anti, got, want)
                            if want:
                                worst = max(worst, abs(got - want) / abs(want))
                        assert st.price == pytest.approx(np.exp(-R * T) * np.mean(x), rel=1e-9, abs=0.0)
    deviation(test="payoffs-vs-rows", model=name, worst_rel=worst, level_clearance=clearance)


# 3 ----------------------------------------------------------------------------------------------------------------------
CELL_STEPS = (2, 4, 5, 13, 64)
CELL_STRIKES = (90.0, 95.0, 100.0, 105.0, 110.0)


@pytest.mark.parametrize("name", list(MODELS))
def test_surface_cells_equal_the_column_payoffs(name):
    model, n = MODELS[name], 64
    order = (3, 0, 4, 2, 1, 3)                        # the caller's order is not the steps' order; step 13 comes twice
    strikes, steps = [CELL_STRIKES[i] for i in order], [CELL_STEPS[i] for i in order]
    strikes[-1] = 97.5
    worst = 0.0
    for N in PATHS:
        both = np.concatenate([device_rows(name, N, n, False)[0], device_rows(name, N, n, True)[0]])
        for is_call in (True, False):
            for anti in (False, True):
                rows = both if anti else both[:N]
                sts = _hip.sabr_surface_prices(F0, T, R, is_call, model, strikes, steps, N, n, SEED, anti)
                assert len(sts) == 6
                for st, strike, m in zip(sts, strikes, steps):
                    x = np.maximum((1.0 if is_call else -1.0) * (rows[:, m] - strike), 0.0)
                    assert st.n == x.size
                    for got, want in ((st.sum, float(np.sum(x))), (st.sumsq, float(np.sum(x * x)))):
                        assert abs(got - want) <= 1e-9 * abs(want), (name, N, is_call, anti, strike, m, got, want)
                        if want:
                            worst = max(worst, abs(got - want) / abs(want))
                    assert st.price == pytest.approx(np.exp(-R * T * m / n) * np.mean(x), rel=1e-9, abs=0.0)
                if N == 257:                           # a cell alone, and beside other neighbours: the same words
                    for j in (0, 2, 5):
                        alone = _hip.sabr_surface_prices(F0, T, R, is_call, model, [strikes[j]], [steps[j]], N, n, SEED, anti)[0]
                        pair = _hip.sabr_surface_prices(F0, T, R, is_call, model, [120.0, strikes[j]], [64, steps[j]], N, n, SEED, anti)[1]
                        assert words(alone) == words(sts[j]) == words(pair), (name, is_call, anti, j)
    deviation(test="surface-vs-columns", model=name, worst_rel=worst)


# 4 ----------------------------------------------------------------------------------------------------------------------
def combined(parts, t):
    return _hip.combine_stats([(p.sum, p.sumsq, p.n) for p in parts], R, t)


@pytest.mark.parametrize("name", list(MODELS))
def test_shards_add_up(name):
    model = MODELS[name]
    for n in (5, 64):
        for anti in (False, True):
            for code in (0, 3, 5, 6, 7, EUROPEAN):
                level = so.level_of(code)
                whole = _hip.sabr_price(F0, K, T, R, True, model, code, level, 257, n, SEED, anti)
                parts = [_hip.sabr_price(F0, K, T, R, True, model, code, level, cnt, n, SEED, anti, path_offset=off) for off, cnt in ((0, 100), (100, 157))]
                assert same(combined(parts, T), whole), (name, n, code, anti)
            steps = [min(m, n) for m in (2, 5, 64)]
            whole = _hip.sabr_surface_prices(F0, T, R, False, model, [95.0, 100.0, 105.0], steps, 257, n, SEED, anti)
            parts = [_hip.sabr_surface_prices(F0, T, R, False, model, [95.0, 100.0, 105.0], steps, cnt, n, SEED, anti, path_offset=off)
                     for off, cnt in ((0, 100), (100, 157))]
            for j, m in enumerate(steps):
                assert same(combined([p[j] for p in parts], T * m / n), whole[j]), (name, n, j, anti)


@pytest.mark.parametrize("name", list(MODELS))
def test_a_shard_beyond_2_to_the_32_equals_the_oracle_s_payoffs(name):
    """The matrices take no offset: the oracle's rows stand in for them.  TIE holds every state within 1e-10 of max(|F|, 1) (test 1), and
    a payoff moves by at most twice the largest move of a state of its path, so a sum by at most 2e-10 sum_paths max_t max(F_t, 1); its
    squares by 2 max(x) times that.  The barrier decisions are the oracle's where no state is within 1e-9 of a level (asserted)."""
    model, N, n, offset = MODELS[name], 63, 13, (1 << 32) + 5
    plain, mirror = oracle(name, N, n, False, offset)[0], oracle(name, N, n, True, offset)[0]
    assert min(oracle(name, N, n, False, offset)[2], oracle(name, N, n, True, offset)[2]) > 1e-7
    both = np.concatenate([plain, mirror]).astype(np.float64)
    assert so.level_clearance(both) > 1e-9
    assert not np.array_equal(plain.astype(np.float64), device_rows(name, 100, 13, False)[0][:N])          # other paths than those at offset 0
    worst = 0.0
    for anti in (False, True):
        rows = both if anti else both[:N]
        slack = 2.0 * TIE["rel"] * float(np.sum(np.max(np.maximum(rows, 1.0), axis=1)))
        for code in range(9):
            for is_call in (True, False):
                x = so.payoffs(rows, code, is_call, K, so.level_of(code))
                st = _hip.sabr_price(F0, K, T, R, is_call, model, code, so.level_of(code), N, n, SEED, anti, path_offset=offset)
                assert st.n == x.size
                worst = max(worst, abs(st.sum - float(np.sum(x))) / slack)
                assert abs(st.sum - float(np.sum(x))) <= slack, (name, code, is_call, anti)
                assert abs(st.sumsq - float(np.sum(x * x))) <= 2.0 * float(np.max(x)) * slack + 1e-300, (name, code, is_call, anti)
        cells = _hip.sabr_surface_prices(F0, T, R, True, model, [0.0, 0.0], [5, 13], N, n, SEED, anti, path_offset=offset)
        for st, m in zip(cells, (5, 13)):
            assert abs(st.sum - float(np.sum(rows[:, m]))) <= slack, (name, m, anti)
    deviation(test="offset-vs-oracle", model=name, worst_of_slack=worst)


@pytest.mark.parametrize("name", list(MODELS))
def test_one_workgroup_walks_every_path_to_the_same_result(name):
    model, N, n = MODELS[name], 4133, 13
    free = {(code, anti): _hip.sabr_price(F0, K, T, R, False, model, code, so.level_of(code), N, n, SEED, anti)
            for code in (1, 4, 6, 7, EUROPEAN) for anti in (False, True)}
    free_cells = _hip.sabr_surface_prices(F0, T, R, True, model, [95.0, 105.0], [5, 13], N, n, SEED, True)
    with grid_cap(1):
        for mirror in (False, True):
            forward, vol = _hip.sabr_paths(F0, T, model, N, n, SEED, mirror=mirror, path_major=True)
            assert np.array_equal(forward, device_rows(name, N, n, mirror)[0]) and np.array_equal(vol, device_rows(name, N, n, mirror)[1])
            f_tm, v_tm = _hip.sabr_paths(F0, T, model, N, n, SEED, mirror=mirror, path_major=False)
            assert np.array_equal(f_tm.T, forward) and np.array_equal(v_tm.T, vol)
        for (code, anti), want in free.items():
            assert same(_hip.sabr_price(F0, K, T, R, False, model, code, so.level_of(code), N, n, SEED, anti), want), (name, code, anti)
        for got, want in zip(_hip.sabr_surface_prices(F0, T, R, True, model, [95.0, 105.0], [5, 13], N, n, SEED, True), free_cells):
            assert same(got, want)


# 5 ----------------------------------------------------------------------------------------------------------------------
def bachelier(F, strike, t, r, sigma, is_call):
    from scipy.special import ndtr

    sd = sigma * math.sqrt(t)
    d = (F - strike) / sd
    sign = 1.0 if is_call else -1.0
    return math.exp(-r * t) * (sign * (F - strike) * ndtr(sign * d) + sd * math.exp(-0.5 * d * d) / math.sqrt(2 * math.pi))


def test_closed_forms_without_vol_of_vol():
    for is_call in (True, False):
        kind = "call" if is_call else "put"
        st = _hip.sabr_price(F0, K, T, R, is_call, (0.25, 1.0, -0.4, 0.0), EUROPEAN, 0.0, 1 << 16, 16, SEED, False)
        black = float(ol.SABRModel._black_price(F0, K, T, R, 0.25, kind))
        deviation(test="black-76", is_call=is_call, price=st.price, closed_form=black, std_errors=abs(st.price - black) / st.std_error)
        assert abs(st.price - black) <= 3.0 * st.std_error
        st = _hip.sabr_price(F0, K, T, R, is_call, (20.0, 0.0, 0.3, 0.0), EUROPEAN, 0.0, 1 << 16, 16, SEED, False)
        normal = bachelier(F0, K, T, R, 20.0, is_call)
        deviation(test="bachelier", is_call=is_call, price=st.price, closed_form=normal, std_errors=abs(st.price - normal) / st.std_error)
        assert abs(st.price - normal) <= 3.0 * st.std_error


# 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,params", [("lognormal-like", (0.2, 1.0, -0.3, 0.4)), ("half", MODELS["half"])])
def test_mild_parameters_agree_with_hagan(name, params):
    assert params[3] == 0.4
    model = ol.SABRModel(*params)
    sts = _hip.sabr_surface_prices(F0, T, R, True, params, [80.0, 100.0, 120.0], [64, 64, 64], 1 << 16, 64, SEED, False)
    for strike, st in zip((80.0, 100.0, 120.0), sts):
        hagan = float(model.price(F0, strike, T, R, "call"))
        deviation(test="hagan", model=name, K=strike, price=st.price, hagan=hagan, std_error=st.std_error, gap=abs(st.price - hagan),
                  bar=3.0 * st.std_error + 0.021)
        assert abs(st.price - hagan) <= 3.0 * st.std_error + 0.021, (name, strike)
        one = _hip.sabr_price(F0, strike, T, R, True, params, EUROPEAN, 0.0, 1 << 16, 64, SEED, False)
        assert one.price == pytest.approx(st.price, rel=1e-9)                                # the surface cell is the one-launch price


# 7 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half", "half-absorbing"])
def test_the_half_kernel_and_the_general_kernel_agree_at_one_half(name):
    alpha, beta, rho, nu = MODELS[name]
    assert beta == 0.5
    beside = (alpha, float(np.nextafter(0.5, 1.0)), rho, nu)
    worst = 0.0
    for N, n in ((257, 13), (4133, 64)):
        for mirror in (False, True):
            half_f, half_v = device_rows(name, N, n, mirror)
            gen_f, gen_v = _hip.sabr_paths(F0, T, beside, N, n, SEED, mirror=mirror, path_major=True)
            assert np.array_equal(half_f == 0.0, gen_f == 0.0), (name, N, n, mirror)
            units = max(tie_units(gen_f, half_f.astype(LONG), 1e-2 * F0), tie_units(gen_v, half_v.astype(LONG)))
            worst = max(worst, units)
            assert units <= 1.0, (name, N, n, mirror, units)
    a = _hip.sabr_price(F0, K, T, R, True, MODELS[name], 6, 0.0, 4133, 64, SEED, True)
    b = _hip.sabr_price(F0, K, T, R, True, beside, 6, 0.0, 4133, 64, SEED, True)
    assert a.sum == pytest.approx(b.sum, rel=1e-9) and a.n == b.n
    deviation(test="half-vs-general", model=name, tie_units=worst, differ=bool(a.sum != b.sum))


# 8 ----------------------------------------------------------------------------------------------------------------------
def test_nan_forward_gives_nan_and_the_next_call_is_right():
    model = MODELS["half"]
    before = _hip.sabr_price(F0, K, T, R, True, model, EUROPEAN, 0.0, 257, 13, SEED, True)
    bad = _hip.sabr_price(float("nan"), K, T, R, True, model, EUROPEAN, 0.0, 257, 13, SEED, True)
    assert np.isnan(bad.price) and np.isnan(bad.std_error) and np.isnan(bad.sum) and bad.n == 514
    assert all(np.isnan(c.price) for c in _hip.sabr_surface_prices(float("nan"), T, R, True, model, [100.0], [13], 257, 13, SEED))
    for m in MODELS.values():
        assert np.isnan(_hip.sabr_paths(float("nan"), T, m, 100, 5, SEED, path_major=True)[0][:, 1:]).all()
    assert np.isnan(_hip.sabr_price(F0, K, T, R, True, (0.2, 0.5, 0.0, float("nan")), 6, 0.0, 100, 5, SEED).price)      # a NaN no check refuses
    after = _hip.sabr_price(F0, K, T, R, True, model, EUROPEAN, 0.0, 257, 13, SEED, True)
    assert words(after) == words(before) and np.isfinite(after.price)


def test_monte_carlo_greeks_through_the_adapter():
    params = (0.2, 1.0, -0.3, 0.4)
    model = ol.SABRModel(*params)
    S, strike, r, q = 100.0, 100.0, R, 0.01
    greeks = ol.compute_greeks_unified(ol.SABRMCAdapter(model, 1 << 14, 16, 7, True), S, strike, T, r, 0.2, "call", q, include_second_order=False)
    assert list(greeks) == ["price", "delta", "gamma", "vega", "theta", "rho"] and all(np.isfinite(v) for v in greeks.values())
    assert greeks["vega"] == 0.0                                                             # sigma is ignored: the bumps share the draws
    forward = S * math.exp((r - q) * T)
    assert greeks["price"] == _hip.sabr_price(forward, strike, T, r, True, params, EUROPEAN, 0.0, 1 << 14, 16, 7, True).price
    h = fd_steps(S)[0]
    deltas = []
    for seed in range(100, 116):
        adapter = ol.SABRMCAdapter(model, 1 << 14, 16, seed, True)
        deltas.append((adapter.price(S + h, strike, T, r, 0.2, "call", q) - adapter.price(S - h, strike, T, r, 0.2, "call", q)) / (2 * h))
    se_fd = float(np.std(deltas, ddof=1))
    hagan = ol.greeks_sabr(model, S, strike, T, r, "call", q)["delta"]
    deviation(test="greeks", delta=greeks["delta"], hagan_delta=hagan, se_fd=se_fd, std_errors=abs(greeks["delta"] - hagan) / se_fd)
    assert se_fd > 0.0 and abs(greeks["delta"] - hagan) <= 3.0 * se_fd


def test_the_python_class_prices_what_the_binding_prices():
    params = MODELS["general"]
    model = ol.SABRModel(*params)
    forward, _vol = model.simulate_paths(F0, T, 4133, 13, 7)
    assert forward.shape == (4133, 14) and np.array_equal(forward, _hip.sabr_paths(F0, T, params, 4133, 13, 7, path_major=True)[0])
    price, err = model.price_monte_carlo(F0, K, T, R, "call", 4133, 13, 7, return_error=True)
    x = np.maximum(forward[:, -1] - K, 0.0)
    assert price == pytest.approx(np.exp(-R * T) * x.mean(), rel=1e-9) and err == pytest.approx(np.exp(-R * T) * x.std() / np.sqrt(4133), rel=1e-9)
    assert model.price_asian(F0, K, T, R, n_paths=4133, n_steps=13, seed=7) == pytest.approx(np.exp(-R * T) * np.maximum(forward[:, 1:].mean(axis=1) - K, 0.0).mean(), rel=1e-9)
    assert model.price_lookback(F0, K, T, R, "put", n_paths=4133, n_steps=13, seed=7) == pytest.approx(
        np.exp(-R * T) * (forward.max(axis=1) - forward[:, -1]).mean(), rel=1e-9)
    alive = forward.max(axis=1) < 125.0
    assert model.price_barrier(F0, K, T, R, 125.0, n_paths=4133, n_steps=13, seed=7) == pytest.approx(np.exp(-R * T) * np.where(alive, x, 0.0).mean(), rel=1e-9)
    strikes = list(np.linspace(70.0, 130.0, 17))                                             # 17 cells: two launches
    surface = model.price_surface(F0, strikes, [5 / 13, 1.0], R, n_paths=4133, n_steps=13, seed=7)
    assert surface.shape == (17, 2)
    assert surface[16, 1] == pytest.approx(np.exp(-R * T) * np.maximum(forward[:, -1] - 130.0, 0.0).mean(), rel=1e-9)
    assert surface[0, 0] == pytest.approx(np.exp(-R * T * 5 / 13) * np.maximum(forward[:, 5] - 70.0, 0.0).mean(), rel=1e-9)
    vols = model.smile_monte_carlo(F0, T, strikes + [1e6], n_paths=1 << 14, n_steps=13, seed=7, antithetic=True)
    assert vols.shape == (18,) and np.all(np.isfinite(vols[:17])) and np.isnan(vols[17])      # no path reaches 1e6: no price, no volatility
    for i, kind in ((0, "put"), (8, "call"), (16, "call")):                                   # out of the money at r = 0: 70 < F <= 100 < 130
        cell = model.price_surface(F0, [strikes[i]], [1.0], 0.0, kind, n_paths=1 << 14, n_steps=13, seed=7, antithetic=True)[0, 0]
        assert vols[i] == ol.implied_volatility(cell, F0, strikes[i], T, 0.0, kind, 0.0)
