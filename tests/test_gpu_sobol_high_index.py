"""Every Sobol kernel tied to SciPy's points deep in the sequence: offsets up to 2^30 - count, aligned and ragged, the carries of
every high Gray bit, the two points per dimension whose integer is 0 (the clip) or 2^30 - 1, and launches long enough to grid-stride.

The reference is tests/sobol_reference.py: points() restates x_t(k) = shift[t] ^ XOR_{b in gray(k)} sv[t][b] in uint64 NumPy
(tests/test_sobol_reference_cpu.py pins it to SciPy's engine, fast-forwarded); SciPy's own fast_forward is linear in offset x d and
would take minutes here.  The payoffs are the oracles of the point-0 tests, fed these normals (z=), at those tests' tolerances:

  terminal prices      rtol 1e-11, atol 0 (test_gpu_parity.py::test_qmc_terminal_array_vs_oracle), the four launch shapes bit-equal
                       (test_gpu_parity.py::test_qmc_block_kernel_equals_the_one_point_kernel and its split sibling);
  european_qmc         price rel 1e-10, std_error rel 1e-9 (test_gpu_parity.py::test_qmc_matches_reference_sobol); the batch answers
                       what european_qmc answers per contract (include/olmc.h), so it takes the same two bars;
  european_qmc_cv      value rel 1e-9 (test_gpu_parity.py::test_qmc_greeks_and_control_variate_run_on_the_same_points);
  Asian/barrier/lookback  price rel 1e-10, abs 1e-12 (test_gpu_exotic_qmc.py::_check_all);
  autocallable/cliquet    price, sum, sumsq rel 1e-10, abs 1e-12 (test_gpu_structured_qmc.py::_tie);
  Heston               sum, sumsq rel 1e-10, abs 1e-12 (test_gpu_heston_qmc.py, test_gpu_heston_path_payoffs.py::TIE; barriers after
                       that file's precondition that no path comes within 1e-9 of a level);
  path matrices        rtol 1e-11; American price rel 1e-9 and the boundary exact on the device's own matrix (test_gpu_american_qmc.py).

olmc_european_qmc_greeks_fd, olmc_asian_qmc_greeks_fd, olmc_extrema_qmc_greeks_fd, olmc_gbm_qmc_paths, olmc_heston_qmc_paths and the
American calls take no point offset in the C ABI: they start at point 0 and are reached here only where a long launch strides.

Every tie prints its worst relative deviation as a `DEVIATION {json}` line (profiles/r13_sobol_high_index.jsonl keeps one run's).
"""
import functools
import json
import math

import numpy as np
import pytest

from optionslab_amd import _hip
from optionslab_amd.exotic import reference_barrier_level
from optionslab_amd.monte_carlo import sobol_tables
from oracle import numpy_reference as orc
from tests import heston_path_oracle as hpo
from tests import sobol_reference as sr
from tests import test_gpu_american_qmc as am
from tests import test_gpu_exotic_qmc as ex
from tests import test_gpu_heston_path_payoffs as hpp
from tests import test_gpu_heston_qmc as hq
from tests import test_gpu_structured_qmc as stq

pytestmark = pytest.mark.gpu

END = 1 << 30
TOP = END - 1
S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.01
KNOBS = (-1, 0, 1, 2)
SEED = 13


def offsets(count):
    """The set O: (class name, first point)."""
    return [("top", END - count), ("2^29", 1 << 29), ("2^29+64", (1 << 29) + 64), ("2^29+4321", (1 << 29) + 4321),
            ("0x2AAAAAAA&~511", 0x2AAAAAAA & ~511), ("0x15555555&~63", 0x15555555 & ~63)]


def carry_ranges():
    """(class, first, count): a ragged and an aligned range across 2^b for every b in 6 .. 29; Gray bits b and b - 1 flip inside."""
    out = []
    for b in range(6, 30):
        for name, half in (("carry-ragged", 70), ("carry-aligned", 512)):
            first, end = max((1 << b) - half, 0), (1 << b) + half             # the low ranges start at point 0
            if end <= END:
                out.append((name, first, end - first))
    return out


_worst = {}


def record(entry, cls, got, want):
    """Keeps and prints the worst relative deviation of an entry point in an offset class."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.where(want != 0, np.abs(want), 1.0)
    dev = float(np.max(np.abs(got - want) / scale)) if want.size else 0.0
    if dev >= _worst.get((entry, cls), -1.0):
        _worst[(entry, cls)] = dev
        print("DEVIATION", json.dumps({"entry": entry, "offsets": cls, "worst_rel": dev}))
    return dev


class knob:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _hip.tune(_hip.TUNE_QMC_BLOCK, self.value)

    def __exit__(self, *exc):
        _hip.tune(_hip.TUNE_QMC_BLOCK, 0)


def tables(d, seed=SEED):
    return sobol_tables(d, seed, END)


def terminal_from_normals(z, antithetic=False):
    """oracle/numpy_reference.py terminal_sobol / terminal_sobol_antithetic (gbm_qmc.py:38-46, :69-76) on given normals."""
    d = z.shape[1]
    dt = T / d
    vol = SIG * np.sqrt(dt)
    if antithetic:
        drift_total = (R - Q - 0.5 * SIG * SIG) * T
        sum_z = vol * np.sum(z, axis=1)
        return np.concatenate([np.exp(np.log(S) + drift_total + sum_z), np.exp(np.log(S) + drift_total - sum_z)])
    drift = (R - Q - 0.5 * SIG * SIG) * dt
    return np.exp(np.log(S) + drift * d + vol * np.sum(z, axis=1))


def check_terminal(d, cls, first, count, sv, shift, antithetic=False):
    want = terminal_from_normals(sr.point_normals(sv, shift, first, count), antithetic)
    got = {}
    for kb in KNOBS:
        with knob(kb):
            got[kb] = _hip.european_qmc_terminal(S, T, R, SIG, Q, count, sv, shift, point_offset=first, antithetic=antithetic)
    record("european_qmc_terminal", cls, got[-1], want)
    for kb in KNOBS:
        assert got[kb].shape == want.shape
        assert np.allclose(got[kb], want, rtol=1e-11, atol=0), (d, cls, first, count, kb, antithetic)
        assert np.array_equal(got[kb], got[-1]), (d, cls, first, count, kb, antithetic)


# ------------------------------------------------------------------------------------------- (a) terminal prices, every form ----
@pytest.mark.parametrize("d", [1, 3, 15, 16, 31, 32, 33, 64, 65, 130, 252])
def test_terminal_prices_deep_in_the_sequence_equal_the_reference_under_every_launch_shape(d):
    sv, shift = tables(d)
    for count in (1, 63, 64, 65, 513, 1000):
        for cls, first in offsets(count):
            check_terminal(d, cls, first, count, sv, shift)
    check_terminal(d, "top", END - 1000, 1000, sv, shift, antithetic=True)          # the mirror, under each knob
    check_terminal(d, "0x2AAAAAAA&~511", 0x2AAAAAAA & ~511, 513, sv, shift, antithetic=True)


@pytest.mark.parametrize("d", [33, 130])
def test_terminal_prices_across_the_carry_of_every_high_gray_bit(d):
    sv, shift = tables(d)
    ranges = carry_ranges()
    assert len(ranges) == 48 and ranges[-1][1] + ranges[-1][2] <= END
    for cls, first, count in ranges:
        check_terminal(d, cls, first, count, sv, shift)


# ------------------------------------------------------------------------------------------------ (b) reduced European sums ----
def payoff(st, strike, is_call):
    return np.maximum(st - strike, 0.0) if is_call else np.maximum(strike - st, 0.0)


def check_stats(st, x, r, T_, label):
    """price rel 1e-10 and std_error rel 1e-9: test_qmc_matches_reference_sobol's bars (monte_carlo.py:145-150: ddof = 0).  sum is the
    price without its constant factor: the same 1e-10; a square doubles a relative error: sumsq 2e-10."""
    disc = math.exp(-r * T_)
    assert st.n == len(x), label
    assert st.price == pytest.approx(float(disc * np.mean(x)), rel=1e-10), label
    assert st.std_error == pytest.approx(float(disc * np.std(x) / np.sqrt(len(x))), rel=1e-9), label
    assert st.sum == pytest.approx(float(np.sum(x)), rel=1e-10), label
    assert st.sumsq == pytest.approx(float(np.sum(x * x)), rel=2e-10), label


@pytest.mark.parametrize("d", [33, 130])
def test_reduced_european_sums_deep_in_the_sequence(d):
    sv, shift = tables(d)
    count = 1000
    rng = np.random.default_rng(d)
    opts = [(float(rng.uniform(90, 110)), float(rng.uniform(90, 110)), float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.0, 0.08)),
             float(rng.uniform(0.15, 0.5)), float(rng.uniform(0.0, 0.03)), bool(i % 2)) for i in range(14)]      # hundreds of points in the money each
    opts[1] = opts[0][:3] + (opts[0][3] + 1e-3,) + opts[0][4:]                    # an r-bump of contract 0: the same vol
    for cls, first in offsets(count):
        z = sr.point_normals(sv, shift, first, count)
        sum_z = np.sum(z, axis=1)
        st_ref = terminal_from_normals(z)
        fwd = S * np.exp((R - Q) * T)
        for kb in KNOBS:
            label = (d, cls, kb)
            with knob(kb):
                call = _hip.european_qmc(S, K, T, R, SIG, Q, True, count, sv, shift, point_offset=first)
                put = _hip.european_qmc(S, K, T, R, SIG, Q, False, count, sv, shift, point_offset=first)
                cv = _hip.european_qmc_cv(S, K, T, R, SIG, Q, False, count, sv, shift, point_offset=first)
                batches = {k: _hip.european_qmc_batch(opts[:k], count, sv, shift, point_offset=first) for k in (2, 8, 14)}
            check_stats(call, payoff(st_ref, K, True), R, T, label + ("call",))
            check_stats(put, payoff(st_ref, K, False), R, T, label + ("put",))
            record("european_qmc", cls, [call.sum, put.sum, call.sumsq], [np.sum(payoff(st_ref, K, True)), np.sum(payoff(st_ref, K, False)),
                                                                          np.sum(payoff(st_ref, K, True) ** 2)])
            # price_with_control_variate (monte_carlo.py:154-186) on the reference's terminal prices
            dd = np.exp(-R * T) * payoff(st_ref, K, False)
            c = np.cov(dd, st_ref)
            beta = c[0, 1] / c[1, 1] if c[1, 1] > 1e-10 else 0.0
            assert cv.n == count
            assert cv.value == pytest.approx(float(np.mean(dd) - beta * (np.mean(st_ref) - fwd)), rel=1e-9), label
            for got, want in ((cv.sum_d, np.sum(dd)), (cv.sum_s, np.sum(st_ref)), (cv.sum_dd, np.sum(dd * dd)), (cv.sum_ss, np.sum(st_ref * st_ref)),
                              (cv.sum_ds, np.sum(dd * st_ref))):
                assert got == pytest.approx(float(want), rel=2e-10), label          # as check_stats: first and second moments
            record("european_qmc_cv", cls, [cv.value, cv.sum_d, cv.sum_ss], [np.mean(dd) - beta * (np.mean(st_ref) - fwd), np.sum(dd), np.sum(st_ref**2)])
            for k, got in batches.items():
                assert len(got) == k
                for (S_, K_, T_, r_, v_, q_, c_), g in zip(opts, got):
                    dt = T_ / d
                    st_o = np.exp(np.log(S_) + (r_ - q_ - 0.5 * v_ * v_) * dt * d + v_ * np.sqrt(dt) * sum_z)
                    check_stats(g, payoff(st_o, K_, c_), r_, T_, label + ("batch", k))
                    record("european_qmc_batch", cls, g.sum, np.sum(payoff(st_o, K_, c_)))


# --------------------------------------------------------------------------------------------------------- (c) path kernels ----
PATH_OFFSETS = [("top", END - 1000), ("2^29+4321", (1 << 29) + 4321), ("0x2AAAAAAA&~511", 0x2AAAAAAA & ~511)]
EX = dict(S=ex.S, T=ex.T, r=ex.R, sigma=ex.SIG, q=ex.Q)
# n -> (autocallable observation frequency, cliquet periods)
STRUCTURED = {1: (1, 1), 3: (2, 3), 50: (10, 7), 252: (21, 12)}


def check_exotics(n, cls, first, count, seed, kinds, constructions=("bridge", "sequential"), legs=(False, True)):
    """asian_qmc / extrema_qmc against test_gpu_exotic_qmc.py's oracle on the normals of points [first, first + count)."""
    sv, shift = tables(n, seed)
    z = sr.point_normals(sv, shift, first, count)
    for construction in constructions:
        bridge = construction == "bridge"
        for antithetic in legs:
            want = ex.oracle_payoffs(n, count, seed, bridge, antithetic, z=z)
            for kind, sub in kinds:
                for ot in ("call", "put"):
                    args = (ex.S, ex.K, ex.T, ex.R, ex.SIG, ex.Q, ot == "call")
                    if kind == "asian":
                        st = _hip.asian_qmc(*args, sub == "geometric", count, sv, shift, bridge, antithetic, first)
                    elif kind == "barrier":
                        level = reference_barrier_level(ex.S, ex.UP if sub.startswith("up") else ex.DOWN, sub)
                        st = _hip.extrema_qmc(*args, _hip.BARRIER_KINDS[sub], level, count, sv, shift, bridge, antithetic, first)
                    else:
                        code = _hip.LOOKBACK_FIXED if sub == "fixed" else _hip.LOOKBACK_FLOATING
                        st = _hip.extrema_qmc(*args, code, 0.0, count, sv, shift, bridge, antithetic, first)
                    x = want[(kind, sub, ot)]
                    price = math.exp(-ex.R * ex.T) * float(np.mean(x))
                    record(f"{kind}_qmc" if kind == "asian" else "extrema_qmc", cls, st.price, price)
                    label = (n, cls, construction, antithetic, kind, sub, ot)
                    assert st.n == len(x), label
                    assert st.price == pytest.approx(price, rel=1e-10, abs=1e-12), label


def check_structured(n, cls, first, count, seed, constructions=("bridge", "sequential"), legs=(False, True)):
    """autocallable_qmc / cliquet_qmc against test_gpu_structured_qmc.py's oracle on the same normals."""
    sv, shift = tables(n, seed)
    freq, periods = STRUCTURED[n]
    jobs = [(stq.auto_payoffs, freq, {}), (stq.cliq_payoffs, periods, {})]
    want = stq.oracle_vectors(n, count, seed, jobs, z=sr.point_normals(sv, shift, first, count))
    for i, (product, par) in enumerate((("auto", freq), ("cliq", periods))):
        for construction in constructions:
            for antithetic in legs:
                x = np.concatenate([want[(i, construction, leg)] for leg in ((0, 1) if antithetic else (0,))])
                st = stq.device_stats(product, par, {}, n, count, seed, construction, antithetic, first)
                label = (product, n, cls, construction, antithetic)
                record("autocallable_qmc" if product == "auto" else "cliquet_qmc", cls, [st.sum, st.sumsq], [np.sum(x), np.sum(x * x)])
                assert st.n == len(x), label
                assert st.price == pytest.approx(stq._price_of(product, x), rel=1e-10, abs=1e-12), label
                assert st.sum == pytest.approx(float(np.sum(x)), rel=1e-10, abs=1e-12), label
                assert st.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10, abs=1e-12), label


def check_heston(n, cls, first, count, seed, model, families, constructions=("bridge", "sequential"), legs=(False, True)):
    """heston_qmc against test_gpu_heston_qmc.py's literal recursion, heston_qmc_path_payoff against tests/heston_path_oracle.py."""
    sv, shift = tables(2 * n, seed)
    z = sr.point_normals(sv, shift, first, count)
    paths = hq.oracle_paths(n, count, seed, model, z=z)
    spots = hpo.sobol_spots(n, count, seed, model, constructions, z=z)
    for construction in constructions:
        assert np.array_equal(spots[(construction, 0)], paths[(construction, 0)][0])          # the two oracles share the market
        if any(family == "barrier" for family, _ in families):
            for leg in (0, 1):
                hpp.assert_clear_of_the_barriers(spots[(construction, leg)], (n, cls, construction, leg))
        for antithetic in legs:
            use = (0, 1) if antithetic else (0,)
            for is_call in (True, False):
                x = np.concatenate([hq.payoffs(paths[(construction, leg)][0], is_call) for leg in use])
                st = hq.device_stats(model, n, count, seed, construction, is_call, antithetic, first)
                label = (n, cls, construction, antithetic, is_call)
                record("heston_qmc", cls, [st.sum, st.sumsq], [np.sum(x), np.sum(x * x)])
                assert st.n == len(x), label
                assert st.sum == pytest.approx(float(np.sum(x)), rel=1e-10, abs=1e-12), label
                assert st.sumsq == pytest.approx(float(np.sum(x * x)), rel=1e-10, abs=1e-12), label
            for family, kind in families:
                for ot in ("call", "put"):
                    x = np.concatenate([hpo.payoffs(spots[(construction, leg)], family, kind, ot) for leg in use])
                    st = hpp.sobol_stats(model, family, kind, ot, count, n, seed, construction, antithetic, first)
                    record("heston_qmc_path_payoff", cls, [st.sum, st.sumsq], [np.sum(x), np.sum(x * x)])
                    hpp.check_sums(st, x, (n, cls, construction, antithetic, family, kind, ot))


EXOTIC_KINDS = [("asian", "arithmetic"), ("asian", "geometric"), ("barrier", "up-and-out"), ("barrier", "down-and-in"), ("lookback", "floating"),
                ("lookback", "fixed")]
HESTON_FAMILIES = [("asian", "arithmetic"), ("barrier", "up-and-out"), ("lookback", "floating")]


@pytest.mark.parametrize("n", [1, 3, 50, 252])
def test_gbm_path_payoffs_deep_in_the_sequence(n):
    for i, (cls, first) in enumerate(PATH_OFFSETS):
        check_exotics(n, cls, first, 1000, (7, 1234, 2**31 - 5)[i], EXOTIC_KINDS)
        check_structured(n, cls, first, 1000, (7, 1234, 2**31 - 5)[i])


@pytest.mark.parametrize("n", [1, 20, 40])
def test_heston_payoffs_deep_in_the_sequence(n):
    assert (hq.S, hq.K, hq.T, hq.R, hq.Q) == (hpo.S, hpo.K, hpo.T, hpo.R, hpo.Q)
    for i, (cls, first) in enumerate(PATH_OFFSETS):
        check_heston(n, cls, first, 1000, (7, 1234, 2**31 - 5)[i], hq.MODELS[i % 2], HESTON_FAMILIES)


# --------------------------------------------------------------------------------------------------------------- (d) the clip ----
@pytest.mark.parametrize("t", [0, 32, 63])
@pytest.mark.parametrize("target", [0, TOP], ids=["x=0", "x=2^30-1"])
def test_the_points_whose_integer_is_0_or_all_ones(t, target):
    """Dimension t of Sobol(64, seed 7) is 0 at one index in 2^30 -- the only uniform the lower clip binds for -- and 2^30 - 1 at one."""
    d, seed = 64, 7
    sv, shift = tables(d, seed)
    k = sr.index_where(np.asarray(sv)[t], shift[t], target)
    assert k is not None
    for first, count in ((k & ~511, 1024), (k - 3, 7)):
        assert 0 <= first and first + count <= END
        x = sr.points(sv, shift, np.arange(first, first + count))
        assert int(x[k - first, t]) == target and np.count_nonzero(x == target) >= 1
        if target == 0:
            assert sr.uniforms(x)[k - first, t] < sr.CLIP and sr.normals(x)[k - first, t] == pytest.approx(-6.3613, abs=1e-4)
        check_terminal(d, "clip", first, count, sv, shift)
        check_exotics(d, "clip", first, count, seed, [("asian", "arithmetic"), ("asian", "geometric")], constructions=("sequential",), legs=(False,))
        check_heston(d // 2, "clip", first, count, seed, hq.USUAL, [], legs=(False,))


# ---------------------------------------------------------------------------------------------------------- (e) grid-striding ----
STRIDE_FIRST = (1 << 29) + 4321


def test_one_point_per_wave_kernels_stride_beyond_8192_workgroups():
    """2 x 32768 + 77 points: the Asian, lookback, autocallable and cliquet launches (four points per workgroup) take three trips."""
    n, count = 3, 2 * 32768 + 77
    check_exotics(n, "stride", STRIDE_FIRST, count, 7, [("asian", "arithmetic"), ("lookback", "floating")], legs=(False,))
    check_structured(n, "stride", STRIDE_FIRST, count, 7, legs=(False,))


def test_heston_launches_stride():
    check_heston(2, "stride", STRIDE_FIRST, (1 << 18) + 77, 1234, hq.USUAL, [], legs=(False,))


LONG, LONG_SEED = (1 << 21) + 67, 7


@functools.lru_cache(maxsize=2)
def long_normals(d):
    """The normals of points [0, 2^21 + 67) in d dimensions, computed once for both constructions and left unchanged."""
    sv, shift = tables(d, LONG_SEED)
    z = sr.point_normals(sv, shift, 0, LONG)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_a_long_gbm_path_matrix_and_the_american_option_on_it(construction):
    """2^21 + 67 points from point 0 (these calls take no offset): lsm_qmc_paths_kernel strides."""
    n, count, bridge = 2, LONG, construction == "bridge"
    Sa, sigma, q, Ka = 100.0, 0.25, 0.01, 100.0
    sv, shift = tables(n, LONG_SEED)
    want = sr.gbm_prices(long_normals(n), bridge, Sa, am.T, am.R, sigma, q)
    pm = _hip.gbm_qmc_paths(Sa, am.T, am.R, sigma, q, count, sv, shift, bridge, path_major=True)
    tm = _hip.gbm_qmc_paths(Sa, am.T, am.R, sigma, q, count, sv, shift, bridge, path_major=False)
    record("gbm_qmc_paths", "stride", pm, want)
    assert pm.shape == (count, n + 1) and np.array_equal(pm, tm.T)
    assert np.allclose(pm, want, rtol=1e-11, atol=0)
    del tm
    # the American price and boundary: the reference's algorithm on the device's own matrix, and the price on the reference's matrix
    pm[:, 0] = am.reference_column0(Sa, count)
    want[:, 0] = am.reference_column0(Sa, count)
    st = _hip.american_lsm_qmc(Sa, Ka, am.T, am.R, sigma, q, False, count, sv, shift, bridge, 3)
    price, x = orc.american_from_paths(pm, Ka, am.T, am.R, "put", 3, return_payoffs=True)
    record("american_lsm_qmc", "stride", [st.sum, st.price], [np.sum(x), price])
    am.assert_tied(st, price, x, am.AMERICAN_TIE)
    assert st.price == pytest.approx(float(orc.american_from_paths(want, Ka, am.T, am.R, "put", 3)), rel=am.AMERICAN_TIE, abs=1e-300)
    b = _hip.exercise_boundary_qmc(Sa, Ka, am.T, am.R, sigma, q, False, count, sv, shift, bridge)
    wb = orc.exercise_boundary_from_paths(pm, Ka, "put")
    assert np.array_equal(b[1:], wb[1:], equal_nan=True)
    assert np.isnan(b[0]) or b[0] == pytest.approx(Sa, rel=1e-14)


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_a_long_heston_path_matrix(construction):
    """2^21 + 67 points, two steps (four dimensions): heston_qmc_paths_kernel strides."""
    n, count, bridge = 2, LONG, construction == "bridge"
    sv, shift = tables(2 * n, LONG_SEED)
    spot_o, var_o = hq.literal_recursion(*hq.step_normals(long_normals(2 * n), construction), hq.USUAL, n)
    spot, var = _hip.heston_qmc_paths(hq.S, hq.T, hq.R, hq.Q, *hq.USUAL, count, sv, shift, bridge, path_major=True)
    spot_t, var_t = _hip.heston_qmc_paths(hq.S, hq.T, hq.R, hq.Q, *hq.USUAL, count, sv, shift, bridge, path_major=False)
    assert np.array_equal(spot_t.T, spot) and np.array_equal(var_t.T, var)
    record("heston_qmc_paths", "stride", spot, spot_o)
    print("heston_qmc_paths variance: worst absolute deviation", float(np.max(np.abs(var - var_o))))
    assert np.allclose(spot, spot_o, rtol=1e-11, atol=0)
    # the variance is truncated at 0 and a difference of terms near it (an error of eps in a normal shows as sigma_v sqrt(v dt) eps,
    # however small the new v): its error is absolute, so the matrix bar 1e-11 is taken of the variance's scale v0 = 0.04 there
    assert np.allclose(var, var_o, rtol=1e-11, atol=1e-11 * hq.USUAL[4])
