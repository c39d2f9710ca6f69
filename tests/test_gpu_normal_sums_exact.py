"""The fp32 chains that sum a path's normals against their exact replay (tests/normal_sum_oracle.py; run with `-m gpu`).

european_path_kernel in every mode, european_multi_kernel, cliquet_kernel and the geometric asian_kernel are held to the sum the
kernels' comments state, replayed bit for bit in NumPy from the device's own transcendentals (the instrumented build's tap of
box_muller_raw and pair_sum_raw on the CPU oracle's Philox words): a constant off in its last digit, an fma split in two, a fold at the
wrong width or a prefix sum kept at another width moves a chain by an fp32 ulp, and that is 850 times the bound here or more
(test_one_ulp_of_a_chain_...).  The 2e-6 of tests/test_gpu_pair_sums.py and tests/test_gpu_parity.py passes all of these.

  terminal prices   |ln(got) - (a +- vol zsum)| <= B = 8 x 2^-52 x max(1, |ln S_T|) for every path and leg
                    (normal_sum_oracle.log_bound derives it), at every branch of the walk and in every launch shape;
  sums              sum and sumsq (the control variate's five moments; every contract of european_multi and of a european_batch of 16)
                    within (2 N - 1) 2^-53 relative of the fp64-exact sums of the oracle's payoffs, N the number of terms, plus B per
                    term; the batch's scaled contracts S_T = exp(a - a_base) S_T,base take two roundings more (10 instead of 8);
  cliquet, Asian    the same on sum and sumsq, with B on every period's logarithm and on the logarithm of the geometric mean.

Every tie prints a line `DEVIATION {json}` before it asserts (pytest -s): the worst ratio to the bound of its family so far.
Measured on an MI355X: the tap returns exactly 1.0 at both unit points and fl32(rad s) is its pair on every pair of every case, so
the factors come from the existing tap alone; worst ratios to the bound: terminal 0.125, european 0.0025, control variate 0.0043,
multi 0.0037, batch 0.0047, cliquet 0.0028, geometric Asian 0.0022; of the 31,137 fp32 chains of the terminal cases none is below
2^-18 and one ulp of any of them is at least 854 B.  The module runs in under two seconds.
"""
import contextlib
import functools
import json
import math

import numpy as np
import pytest

from optionslab_amd import _hip
from tests import normal_sum_oracle as nso
from tests.gpu_support import device_fixture

pytestmark = pytest.mark.gpu

LONG = np.longdouble
DEFAULTS = {_hip.TUNE_SPLIT_TAIL: 0, _hip.TUNE_PHILOX_TABLE: 1, _hip.TUNE_GRID_CAP: 0}
SHAPES = {"default": {}, "whole_workgroups": {_hip.TUNE_SPLIT_TAIL: -1}, "no_table": {_hip.TUNE_PHILOX_TABLE: 0},
          "whole_no_table": {_hip.TUNE_SPLIT_TAIL: -1, _hip.TUNE_PHILOX_TABLE: 0}, "grid_cap_1": {_hip.TUNE_GRID_CAP: 1}}
WORST = {}


def _restore():
    for knob, value in DEFAULTS.items():
        _hip.tune(knob, value)


_device = device_fixture(after=_restore)


def TAP(xa, xb):
    from tools.probe import binding as probe

    return probe.box_muller_probe(xa, xb)


@contextlib.contextmanager
def knobs(setting):
    try:
        for knob, value in setting.items():
            _hip.tune(knob, value)
        yield
    finally:
        _restore()


def deviation(family, case, of_bound):
    WORST[family] = max(WORST.get(family, 0.0), float(of_bound))
    print("DEVIATION " + json.dumps(dict(family=family, case=[str(c) for c in case], of_bound=float(of_bound), worst=WORST[family])))


@functools.lru_cache(maxsize=None)
def drawn(path_offset, count, blocks, tag=0):
    """(words, factors) of a case, the factors accepted by both checks of normal_sum_oracle.pair_factors on every pair."""
    words = nso.case_words(nso.SEED, path_offset, count, blocks, tag)
    return words, nso.block_factors(TAP, words)


def exp_error(log_value, units=8.0):
    """What the bound on a logarithm allows on its exponential, relative: e^B - 1."""
    return np.expm1(units / 8.0 * nso.log_bound(log_value))


def hold_moment(label, got, terms, allowed, extra_roundings=0):
    """got against the sum of `terms` (np.longdouble) within (2 N - 1 + extra) 2^-53 relative plus `allowed` per term; the ratio."""
    n = terms.size
    want = terms.sum()
    bound = (2 * n - 1 + extra_roundings) * 2.0 ** -53 * float(np.abs(terms).sum()) + float(np.sum(allowed))
    ratio = abs(float(LONG(got) - want)) / bound
    return ratio, (label, got, float(want), bound)


def hold_sums(family, case, got_sum, got_sumsq, x, dx, extra_roundings=0):
    a, why_a = hold_moment("sum", got_sum, x, dx, extra_roundings)
    b, why_b = hold_moment("sumsq", got_sumsq, x * x, (2.0 * np.abs(x) * dx + dx * dx).astype(np.float64), extra_roundings)
    deviation(family, case, max(a, b))
    assert a <= 1.0, (case, why_a)
    assert b <= 1.0, (case, why_b)


# ------------------------------------------------------------------------------------------------- the instruments ----
def test_the_tap_returns_one_at_the_unit_points_and_the_words_are_the_devices():
    assert nso.tap_at_the_unit_points(TAP) == (1.0, 1.0)
    for offset, count, tag in ((0, nso.TERMINAL_PATHS, 0), (nso.SUM_OFFSET, nso.SUM_PATHS, 0), (0, nso.SUM_PATHS, 0xFFFFFFFF)):
        assert np.array_equal(_hip.philox_words(nso.SEED, offset, count, 0, 9, tag), nso.case_words(nso.SEED, offset, count, 9, tag))
    paths, n_steps = nso.MIXED_SHAPE
    assert np.array_equal(_hip.philox_words(nso.SEED, 0, paths, 0, nso.blocks_of(n_steps)), nso.case_words(nso.SEED, 0, paths, nso.blocks_of(n_steps)))


def test_one_ulp_of_a_chain_is_a_hundred_times_the_bound_on_the_devices_factors():
    """tests/test_normal_sum_oracle_cpu.py's resolution, on the factors the device returned."""
    words, f = drawn(0, nso.TERMINAL_PATHS, nso.blocks_of(max(nso.TERMINAL_STEPS)))
    small_all, total_all, least_all = 0, 0, math.inf
    for n_steps in nso.TERMINAL_STEPS:
        chains = []
        zsum = nso.european_zsum(words, n_steps, f, chains)
        a, vol = nso.contract(n_steps=n_steps, **nso.TERMINAL)
        small, total, least = nso.resolution(chains, vol, np.stack([a + vol * zsum, a - vol * zsum]))
        small_all, total_all, least_all = small_all + small, total_all + total, min(least_all, least)
        assert small * 10_000 <= total, (n_steps, small, total)
        assert least >= 100.0, (n_steps, least)
    print("RESOLUTION " + json.dumps(dict(chains=total_all, below_2_to_minus_18=small_all, least_ulp_over_bound=least_all)))


# ------------------------------------------------------------------------------------------------- terminal prices ----
def hold_terminal(case, paths, n_steps, words, f):
    p = nso.TERMINAL
    a, vol = nso.contract(n_steps=n_steps, **p)
    zsum = nso.european_zsum(words, n_steps, f).astype(LONG)
    plain, mirror = LONG(a) + LONG(vol) * zsum, LONG(a) - LONG(vol) * zsum
    for antithetic in (False, True):
        got = _hip.european_terminal(p["S"], p["T"], p["r"], p["sigma"], p["q"], paths, n_steps, nso.SEED, antithetic)
        want = np.concatenate([plain, mirror]) if antithetic else plain
        assert got.shape == want.shape and np.all(got > 0.0) and np.isfinite(got).all(), case
        dev = np.abs((np.log(got.astype(LONG)) - want).astype(np.float64))
        bound = nso.log_bound(want.astype(np.float64))
        deviation("terminal", (*case, antithetic), np.max(dev / bound))
        worst = int(np.argmax(dev / bound))
        assert np.all(dev <= bound), (case, antithetic, worst % paths, float(dev[worst]), float(bound[worst]))


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n_steps", nso.TERMINAL_STEPS)
def test_terminal_prices_are_the_replayed_sum_in_every_launch_shape(n_steps, shape):
    words, f = drawn(0, nso.TERMINAL_PATHS, nso.blocks_of(max(nso.TERMINAL_STEPS)))
    with knobs(SHAPES[shape]):
        hold_terminal((shape, n_steps), nso.TERMINAL_PATHS, n_steps, words, f)


def test_terminal_prices_of_a_launch_that_mixes_whole_and_split_workgroups():
    """65,636 paths: on 256 compute units 256 whole workgroups and two split ones (36 live lanes in the last) in one launch."""
    paths, n_steps = nso.MIXED_SHAPE
    words, f = drawn(0, paths, nso.blocks_of(n_steps))
    hold_terminal(("mixed", n_steps), paths, n_steps, words, f)


# ------------------------------------------------------------------------------------------------------------ sums ----
def payoffs(a, vol, zsum, strike, antithetic, units=8.0):
    """(x, dx): the call's payoffs S_T - K of the plain leg, then of the mirrored one, and what the bound allows on each."""
    z = zsum.astype(LONG)
    logs = np.concatenate([LONG(a) + LONG(vol) * z, LONG(a) - LONG(vol) * z]) if antithetic else LONG(a) + LONG(vol) * z
    spot = np.exp(logs)
    assert np.all(spot > 2.0 * strike)                                              # deep in the money: nothing clips
    return spot - LONG(strike), (spot * exp_error(logs.astype(np.float64), units)).astype(np.float64), spot


@pytest.mark.parametrize("antithetic", [False, True])
@pytest.mark.parametrize("n_steps", nso.SUM_STEPS)
def test_european_sums_beyond_2_to_the_32(n_steps, antithetic):
    p = nso.SUMS
    words, f = drawn(nso.SUM_OFFSET, nso.SUM_PATHS, nso.blocks_of(max(nso.SUM_STEPS)))
    a, vol = nso.contract(p["S"], p["T"], p["r"], p["sigma"], p["q"], n_steps)
    x, dx, _spot = payoffs(a, vol, nso.european_zsum(words, n_steps, f), p["K"], antithetic)
    st = _hip.european(p["S"], p["K"], p["T"], p["r"], p["sigma"], p["q"], True, nso.SUM_PATHS, n_steps, nso.SEED, antithetic, path_offset=nso.SUM_OFFSET)
    assert st.n == x.size
    hold_sums("european", (n_steps, antithetic), st.sum, st.sumsq, x, dx)


@pytest.mark.parametrize("antithetic", [False, True])
@pytest.mark.parametrize("n_steps", nso.SUM_STEPS)
def test_control_variate_moments(n_steps, antithetic):
    """sum x, sum S_T, sum x^2, sum S_T^2, sum x S_T; the host discounts the payoff's (disc, disc^2, disc: up to four roundings more)."""
    p = nso.SUMS
    words, f = drawn(0, nso.SUM_PATHS, nso.blocks_of(max(nso.SUM_STEPS)))
    a, vol = nso.contract(p["S"], p["T"], p["r"], p["sigma"], p["q"], n_steps)
    x, dx, spot = payoffs(a, vol, nso.european_zsum(words, n_steps, f), p["K"], antithetic)
    got = _hip.european_cv(p["S"], p["K"], p["T"], p["r"], p["sigma"], p["q"], True, nso.SUM_PATHS, n_steps, nso.SEED, antithetic)
    assert got.n == x.size
    disc = LONG(math.exp(-p["r"] * p["T"]))
    both = (dx * dx).astype(np.float64)
    moments = (("sum_d", got.sum_d, disc * x, float(disc) * dx), ("sum_s", got.sum_s, spot, dx),
               ("sum_dd", got.sum_dd, disc * disc * x * x, float(disc * disc) * (2.0 * np.abs(x) * dx + both).astype(np.float64)),
               ("sum_ss", got.sum_ss, spot * spot, (2.0 * spot * dx + both).astype(np.float64)),
               ("sum_ds", got.sum_ds, disc * x * spot, float(disc) * ((np.abs(x) + spot) * dx + both).astype(np.float64)))
    ratios = {}
    for name, value, terms, allowed in moments:
        ratios[name], why = hold_moment(name, value, terms, allowed, extra_roundings=4)
        assert ratios[name] <= 1.0, (n_steps, antithetic, why)
    deviation("control_variate", (n_steps, antithetic), max(ratios.values()))


@pytest.mark.parametrize("antithetic", [False, True])
@pytest.mark.parametrize("n_steps", nso.SUM_STEPS)
def test_european_multi_sums_on_every_tag(n_steps, antithetic):
    """One launch of four contracts, each on its own stream: the tag is counter word 3."""
    p = nso.SUMS
    spots = [p["S"], 90.0, 120.0, 75.0]
    out = _hip.european_multi(spots, p["K"], p["T"], p["r"], p["sigma"], p["q"], True, nso.SUM_PATHS, n_steps, nso.SEED, antithetic,
                              tags=list(nso.MULTI_TAGS))
    for j, tag in enumerate(nso.MULTI_TAGS):
        words, f = drawn(0, nso.SUM_PATHS, nso.blocks_of(max(nso.SUM_STEPS)), tag)
        a, vol = nso.contract(spots[j], p["T"], p["r"], p["sigma"], p["q"], n_steps)
        x, dx, _spot = payoffs(a, vol, nso.european_zsum(words, n_steps, f), p["K"], antithetic)
        assert int(out["n"][j]) == x.size
        hold_sums("multi", (n_steps, antithetic, tag), float(out["sum"][j]), float(out["sumsq"][j]), x, dx)


BATCH = [(s0, nso.SUMS["K"], nso.SUMS["T"], rate, sigma, nso.SUMS["q"], True)
         for sigma in (0.2, 0.15, 0.3, 0.1) for s0, rate in ((100.0, 0.05), (101.0, 0.05), (100.0, 0.06), (93.0, 0.02))]


@pytest.mark.parametrize("antithetic", [False, True])
@pytest.mark.parametrize("n_steps", nso.SUM_STEPS)
def test_a_batch_of_sixteen_contracts_in_four_volatility_groups(n_steps, antithetic):
    """The fused set: one base per volatility (two where a group straddles the middle of the set), the others exp(a - a_base) times its
    terminal prices -- the rounding of a - a_base, of its exponential and of the product: 10 x 2^-52 instead of 8."""
    words, f = drawn(nso.SUM_OFFSET, nso.SUM_PATHS, nso.blocks_of(max(nso.SUM_STEPS)))
    zsum = nso.european_zsum(words, n_steps, f)
    nsets, _pos, mask, _cont, _scale = _hip.contract_layout(BATCH, n_steps)
    assert nsets == 16 and 4 <= bin(mask).count("1") <= 5
    out = _hip.european_batch(BATCH, nso.SUM_PATHS, n_steps, nso.SEED, antithetic, path_offset=nso.SUM_OFFSET)
    for j, (s0, strike, t_end, rate, sigma, q, _call) in enumerate(BATCH):
        a, vol = nso.contract(s0, t_end, rate, sigma, q, n_steps)
        x, dx, _spot = payoffs(a, vol, zsum, strike, antithetic, units=10.0)
        assert out[j].n == x.size
        hold_sums("batch", (n_steps, antithetic, j), out[j].sum, out[j].sumsq, x, dx)


# --------------------------------------------------------------------------------------------------------- cliquet ----
@pytest.mark.parametrize("antithetic", [False, True])
@pytest.mark.parametrize("trailing", nso.CLIQUET_TRAILING)
@pytest.mark.parametrize("steps_per_period", nso.CLIQUET_STEPS_PER_PERIOD)
def test_cliquet_sums(steps_per_period, trailing, antithetic):
    """x = S sum_k (exp(period_drift +- vol psum_k) - 1): no clip binds and every total is positive (asserted, not masked)."""
    p = nso.CLIQUET
    periods = nso.CLIQUET_PERIODS
    n_steps = periods * steps_per_period + trailing
    words, f = drawn(nso.SUM_OFFSET, nso.SUM_PATHS, nso.blocks_of(max(nso.SUM_STEPS)))
    psum = nso.cliquet_period_sums(words, n_steps, periods, f, f.normals).astype(LONG)
    _dt, drift, vol = nso.gbm_step(p["T"], n_steps, p["r"], p["q"], p["sigma"])
    vol, period_drift = vol * nso.Z_SCALE, steps_per_period * drift
    y = np.concatenate([LONG(period_drift) + LONG(vol) * psum, LONG(period_drift) - LONG(vol) * psum]) if antithetic else LONG(period_drift) + LONG(vol) * psum
    local = np.expm1(y)
    assert np.all(local > p["local_floor"]) and np.all(local < p["local_cap"])
    total = local.sum(axis=1)
    assert np.all(total > 0.0) and np.all(total < p["global_cap"])
    x = total * LONG(p["S"])
    dx = p["S"] * np.sum(np.exp(y) * exp_error(y.astype(np.float64)), axis=1).astype(np.float64)
    st = _hip.cliquet(p["S"], p["T"], p["r"], p["sigma"], p["q"], p["local_cap"], p["local_floor"], p["global_cap"], p["global_floor"], periods,
                      nso.SUM_PATHS, n_steps, nso.SEED, antithetic, path_offset=nso.SUM_OFFSET)
    assert st.n == x.size
    hold_sums("cliquet", (steps_per_period, trailing, antithetic), st.sum, st.sumsq, x, dx)


# ------------------------------------------------------------------------------------------------- geometric Asian ----
@pytest.mark.parametrize("antithetic", [False, True])
@pytest.mark.parametrize("n_steps", nso.ASIAN_STEPS)
def test_geometric_asian_sums(n_steps, antithetic):
    """x = exp(ln S + run / M) - K, run the kernel's own sum over the dates of ln(S_t / S)."""
    p = nso.SUMS
    words, f = drawn(nso.SUM_OFFSET, nso.SUM_PATHS, nso.blocks_of(max(nso.SUM_STEPS)))
    _dt, drift, vol = nso.gbm_step(p["T"], n_steps, p["r"], p["q"], p["sigma"])
    run_u, run_d = nso.geometric_asian_run(words, n_steps, f.normals, vol * nso.Z_SCALE, drift)
    run = np.concatenate([run_u, run_d]) if antithetic else run_u
    logs = LONG(math.log(p["S"])) + run.astype(LONG) / LONG(n_steps)
    mean = np.exp(logs)
    assert np.all(mean > 2.0 * p["K"])
    x, dx = mean - LONG(p["K"]), (mean * exp_error(logs.astype(np.float64))).astype(np.float64)
    st = _hip.asian(p["S"], p["K"], p["T"], p["r"], p["sigma"], p["q"], True, True, nso.SUM_PATHS, n_steps, nso.SEED, antithetic, nso.SUM_OFFSET)
    assert st.n == x.size
    hold_sums("asian", (n_steps, antithetic), st.sum, st.sumsq, x, dx)
