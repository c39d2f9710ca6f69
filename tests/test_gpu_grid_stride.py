"""Every path kernel's grid-stride trips, taken at small sizes under OLMC_TUNE_GRID_CAP (include/olmc.h: the launch shape changes,
no result does).  Uncapped, a Philox thread takes a second path only beyond 2^26 paths and a Sobol wave a second point or block only
beyond 2^15 points (2 x CUs x 256 points for the Heston bridge slabs); under a cap of 1, 2 or 3 workgroups they do at a few hundred.

Philox (caps 1 and 3; N = 257 / 769: exactly one thread owns a second path under cap 1 / 3; N = 2000 under cap 3: three trips, the
last one ragged inside a wave):
  * n is equal, and every sum and sum of squares equals the uncapped launch's to the reassociation of two rounded fp64 sums of the
    same n_terms = paths x legs non-negative terms: each is within gamma = n u / (1 - n u) (u = 2^-53) of the exact sum E, so they
    differ by at most 2 gamma E <= 2 gamma / (1 - gamma) of either -- 2 n 2^-53 to first order; computed below (bound()), nothing
    hard-coded.  For the American price this also means the same exercise decisions (a flipped one moves a sum by a cash flow).
  * where oracle/philox_oracle.py restates the entry point, the capped result meets it at test_gpu_property.py's bar (close(), REL
    and the scales per entry point, restated here).
  * per-path outputs are byte-identical, in both layouts; the fused entry points that keep their grid return the same bits.
Sobol (cap 2, 1000 points: 125 trips of a wave-per-point kernel, two trips -- the second ragged -- of a block kernel, each wave's
bridge row or slab reused): the oracles and bars of tests/test_gpu_sobol_high_index.py and of the Heston modules, unchanged.

Every tie prints its worst deviation as a `DEVIATION {json}` line (profiles/r19_grid_stride.jsonl keeps one run's).
"""
import contextlib
import json
import math

import numpy as np
import pytest

from optionslab_amd import _hip
from optionslab_amd.monte_carlo import sobol_tables
from oracle import numpy_reference as orc
from oracle import philox_oracle as po
from tests import heston_path_oracle as hpo
from tests import heston_qe_reference as qe
from tests import sobol_reference as sr
from tests import test_gpu_american_qmc as am
from tests import test_gpu_exotic_qmc_greeks as xg
from tests import test_gpu_heston_qe as hqe
from tests import test_gpu_heston_qmc as hq
from tests import test_gpu_heston_scenarios as hsc
from tests import test_gpu_heston_structured as hst
from tests import test_gpu_heston_surface as hsf
from tests import test_gpu_sobol_high_index as hi

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]        # SciPy: 1000 is not a power of two

REL = 2e-6                                        # test_gpu_property.py
CAPS = (1, 3)
PATHS = (257, 769, 2000)
STEPS = (5, 67, 130)
EUROPEAN_STEPS = STEPS + (252, 257)               # 257 steps are 65 Philox blocks: beyond the prefix table
OFFSETS = (0, 2**32 - 100)                        # the second: the high path word changes inside every launch
SEED = (0x9E3779B9 << 32) | 20240229              # a non-zero high key word
S, K, T, R, SIG, Q = 100.0, 105.0, 1.0, 0.05, 0.2, 0.01
HESTON = hpo.USUAL
MERTON, KOU = (False, 1.0, -0.1, 0.2, 0.0), (True, 1.0, 0.4, 10.0, 5.0)
AUTOCALL = (1.0, 0.9, 0.1, 0.8)                   # autocall level, coupon level, coupon rate, knock-in level
CLIQUET = (0.05, -0.05, 0.5, 0.0)                 # local cap, local floor, global cap, global floor
OBSERVATION_FREQ = {5: 2, 67: 21, 130: 21}
PERIODS = {5: 5, 67: 4, 130: 12}
SOBOL_CAP, SOBOL_POINTS = 2, 1000
SOBOL_FIRSTS = (("0", 0), ("2^29+4321", (1 << 29) + 4321))


@contextlib.contextmanager
def grid_cap(value):
    """The knob is process-global: 0 again whatever happens inside."""
    _hip.tune(_hip.TUNE_GRID_CAP, value)
    try:
        yield
    finally:
        _hip.tune(_hip.TUNE_GRID_CAP, 0)


def close(a, b, scale=1.0, n=0, level=0.0, power=1):
    """test_gpu_property.py's rule: relative 2e-6 of the sum -- or, when the sum is small because most payoffs sit near / below their
    kink, the absolute error that n prices of size `level`, each good to 2e-6 relative (hardware log2 / sin / cos), can leave."""
    return a == pytest.approx(b, rel=REL * scale, abs=1e-9 * scale + REL * scale * n * (3.0 * level) ** power)


def bound(n_terms):
    """Two rounded fp64 sums of the same n_terms non-negative terms, relative to either of them (module docstring)."""
    gamma = n_terms * 2.0**-53 / (1.0 - n_terms * 2.0**-53)
    return 2.0 * gamma / (1.0 - gamma)


_worst = {}


def record(entry, what, value):
    if value >= _worst.get((entry, what), -1.0):
        _worst[(entry, what)] = value
        print("DEVIATION", json.dumps({"entry": entry, "what": what, "worst": value}))


def sums_of(result):
    """(n, [sums]) of a Stats, a CvMoments or a list of Stats."""
    if isinstance(result, (list, tuple)):
        parts = [sums_of(r) for r in result]
        assert len({n for n, _ in parts}) == 1
        return parts[0][0], [x for _, xs in parts for x in xs]
    if hasattr(result, "sum_d"):
        return result.n, [result.sum_d, result.sum_s, result.sum_dd, result.sum_ss, result.sum_ds]
    return result.n, [result.sum, result.sumsq]


def assert_same_sums(entry, capped, plain, label):
    """The capped launch's n and sums against the uncapped launch's, to bound(n)."""
    (n_c, got), (n_p, want) = sums_of(capped), sums_of(plain)
    assert n_c == n_p and len(got) == len(want), label
    tol = bound(n_p)
    for i, (g, w) in enumerate(zip(got, want)):
        assert math.isfinite(w) and w >= 0.0, (label, i, w)
        record(entry, "capped vs uncapped, in units of the bound", abs(g - w) / (tol * w) if w > 0.0 else float(g != w))
        assert abs(g - w) <= tol * w, (label, i, g, w, tol)


def assert_close(entry, ok, got, want, label):
    record(entry, "capped vs checker, relative", abs(got - want) / abs(want) if want else abs(got))
    assert ok, (label, got, want)


def shapes(steps=STEPS, offsets=OFFSETS, antithetic=(False, True)):
    return [(N, M, anti, off) for N in PATHS for M in steps for anti in antithetic for off in offsets]


def sweep(entry, call, check=None, **kw):
    """call(N, M, anti, off) uncapped and under each cap; check(result, N, M, anti, off, label) holds the capped result to the checker
    (its reference computed once per shape: memoise in the caller)."""
    for N, M, anti, off in shapes(**kw):
        plain = call(N, M, anti, off)
        for cap in CAPS:
            label = (entry, N, M, anti, off, cap)
            with grid_cap(cap):
                capped = call(N, M, anti, off)
            assert_same_sums(entry, capped, plain, label)
            if check is not None:
                check(capped, N, M, anti, off, label)


def memo(f):
    cache = {}

    def g(*a):
        if a not in cache:
            cache[a] = f(*a)
        return cache[a]
    return g


def check_two(entry, st, want, scale, level, label):
    """sum at `scale`, sumsq at 4 x scale with the squared level: the pattern of every one-contract bar in test_gpu_property.py."""
    sx, sxx, n = want
    assert st.n == n, label
    assert_close(entry, close(st.sum, sx, scale, n, level), st.sum, sx, label)
    assert_close(entry, close(st.sumsq, sxx, 4 * scale, n, level, 2), st.sumsq, sxx, label)


# ============================================================================================================== Philox ====
@pytest.mark.parametrize("is_call", [True, False])
def test_european_and_its_control_variate_moments(is_call):
    want = memo(lambda N, M, anti, off: po.european_moments(S, K, T, R, SIG, Q, is_call, N, M, SEED, anti, off))

    def check(st, N, M, anti, off, label):
        sx, sxx, *_rest, n = want(N, M, anti, off)
        check_two("european", st, (sx, sxx, n), 1, max(S, K), label)

    sweep("european", lambda N, M, anti, off: _hip.european(S, K, T, R, SIG, Q, is_call, N, M, SEED, anti, path_offset=off), check,
          steps=EUROPEAN_STEPS)

    def check_cv(cv, N, M, anti, off, label):
        sx, sxx, ss, sss, sxs, n = want(N, M, anti, off)
        disc, level = math.exp(-R * T), max(S, K) * math.exp(3 * SIG * math.sqrt(T))
        assert cv.n == n, label
        for got, ref, scale, power in ((cv.sum_d, disc * sx, 1, 1), (cv.sum_dd, disc * disc * sxx, 4, 2), (cv.sum_s, ss, 1, 1),
                                       (cv.sum_ss, sss, 4, 2), (cv.sum_ds, disc * sxs, 4, 2)):
            assert_close("european_cv_shard", close(got, ref, scale, n, level, power), got, ref, label)

    sweep("european_cv_shard", lambda N, M, anti, off: _hip.european_cv_shard(S, K, T, R, SIG, Q, is_call, off, N, M, SEED, anti), check_cv,
          steps=EUROPEAN_STEPS)


@pytest.mark.parametrize("k", [8, 14])
def test_european_batch(k):
    """8 and 14 contracts: the 8- and 16-slot kernels, strided.  Groups of equal vol (one base, scaled followers), calls and puts."""
    opts = [(S + 0.5 * (i % 3), K - 2.0 * (i % 5), T, R + 1e-3 * (i % 2), 0.15 + 0.05 * (i % 4), Q, i % 3 != 1) for i in range(k)]
    want = memo(lambda i, N, M, anti, off: po.european_moments(*opts[i][:6], opts[i][6], N, M, SEED, anti, off))

    def check(stats, N, M, anti, off, label):
        assert len(stats) == k
        for i, st in enumerate(stats):
            sx, sxx, *_rest, n = want(i, N, M, anti, off)
            check_two("european_batch", st, (sx, sxx, n), 1, max(opts[i][0], opts[i][1]), label + (i,))

    sweep("european_batch", lambda N, M, anti, off: _hip.european_batch(opts, N, M, SEED, anti, path_offset=off), check, steps=EUROPEAN_STEPS)


@pytest.mark.parametrize("kind", ["geometric", "arithmetic", "fast"])
def test_asian(kind):
    geo, fast = kind == "geometric", kind == "fast"
    want = memo(lambda N, M, anti, off: po.asian_moments(S, K, T, R, SIG, Q, True, geo, N, M, SEED, anti, off))
    sweep("asian " + kind, lambda N, M, anti, off: _hip.asian(S, K, T, R, SIG, Q, True, geo, N, M, SEED, anti, path_offset=off, fast=fast),
          lambda st, N, M, anti, off, label: check_two("asian " + kind, st, want(N, M, anti, off), 1, max(S, K), label))


@pytest.mark.parametrize("payoff,level", [(0, 125.0), (3, 90.0), (4, 0.0), (5, 0.0)], ids=["up-and-out", "down-and-in", "floating", "fixed"])
def test_barrier_and_lookback(payoff, level):
    want = memo(lambda N, M, anti, off: po.extrema_moments(S, K, T, R, SIG, Q, True, payoff, level, N, M, SEED, anti, off))
    if payoff < 4:
        entry, lvl = "barrier", max(S, K) * math.exp(3 * SIG * math.sqrt(T))
        call = lambda N, M, anti, off: _hip.barrier(S, K, T, R, SIG, Q, True, level, payoff, N, M, SEED, anti, path_offset=off)
    else:
        entry, lvl = "lookback", max(S, K)
        call = lambda N, M, anti, off: _hip.lookback(S, K, T, R, SIG, Q, True, payoff == 5, N, M, SEED, anti, path_offset=off)
    sweep(entry, call, lambda st, N, M, anti, off, label: check_two(entry, st, want(N, M, anti, off), 1, lvl, label))


def test_autocallable_and_cliquet():
    want_a = memo(lambda N, M, anti, off: po.autocall_moments(S, T, R, SIG, Q, *AUTOCALL, OBSERVATION_FREQ[M], N, M, SEED, anti, off))
    sweep("autocallable", lambda N, M, anti, off: _hip.autocallable(S, T, R, SIG, Q, *AUTOCALL, OBSERVATION_FREQ[M], N, M, SEED, anti, path_offset=off),
          lambda st, N, M, anti, off, label: check_two("autocallable", st, want_a(N, M, anti, off), 1, 1.0, label))
    want_c = memo(lambda N, M, anti, off: po.cliquet_moments(S, T, R, SIG, Q, *CLIQUET, PERIODS[M], N, M, SEED, anti, off))
    sweep("cliquet", lambda N, M, anti, off: _hip.cliquet(S, T, R, SIG, Q, *CLIQUET, PERIODS[M], N, M, SEED, anti, path_offset=off),
          lambda st, N, M, anti, off, label: check_two("cliquet", st, want_c(N, M, anti, off), 1, S, label))


def test_heston_and_jump_diffusion():
    want_h = memo(lambda N, M, anti, off: po.heston_moments(S, K, T, R, Q, True, *HESTON, N, M, SEED, anti, off))
    sweep("heston", lambda N, M, anti, off: _hip.heston(S, K, T, R, Q, True, *HESTON, N, M, SEED, anti, path_offset=off),
          lambda st, N, M, anti, off, label: check_two("heston", st, want_h(N, M, anti, off), 2, max(S, K), label))
    for name, model in (("merton", MERTON), ("kou", KOU)):
        want_j = memo(lambda N, M, anti, off: po.jump_moments(S, K, T, R, SIG, Q, True, *model, N, M, SEED, off))
        sweep("jump_diffusion " + name, lambda N, M, anti, off: _hip.jump_diffusion(S, K, T, R, SIG, Q, True, *model, N, M, SEED, path_offset=off),
              lambda st, N, M, anti, off, label: check_two("jump_diffusion " + name, st, want_j(N, M, anti, off), 2, max(S, K), label),
              antithetic=(False,))


@pytest.mark.parametrize("family,kind", [("asian", "arithmetic"), ("barrier", "up-and-out"), ("lookback", "floating")])
def test_heston_path_payoff(family, kind):
    code, level = hpo.payoff_code(family, kind)
    sweep("heston_path_payoff " + family,
          lambda N, M, anti, off: _hip.heston_path_payoff(S, K, T, R, Q, True, *HESTON, code, level, N, M, SEED, anti, off))


def surface_cells(M):
    """(strike, step), unsorted: the first and the last step, steps inside a Philox block of the Euler walk (two steps per block) and on
    both sides of a block boundary, an interior step past 64 and 128 where there is one."""
    return [(100.0, M), (80.0, 1), (120.0, M), (100.0, 2), (90.0, 3), (110.0, M - 1), (100.0, M // 2 + 1), (95.0, 4)]


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_heston_surfaces(scheme):
    launch = _hip.heston_surface if scheme == "euler" else _hip.heston_qe_surface
    model = HESTON if scheme == "euler" else qe.STEEP

    def call(N, M, anti, off):
        cells = surface_cells(M)
        return launch(S, T, R, Q, True, *model, [k for k, _ in cells], [m for _, m in cells], N, M, SEED, anti, off)

    sweep("heston_surface " + scheme, call)


def test_heston_scenarios():
    """16 scenarios of 6 recursions, one of them from v0 < 0 (test_gpu_heston_scenarios.py's MIXED set)."""
    scenarios = hsc.mixed_set(HESTON)
    sweep("heston_scenarios", lambda N, M, anti, off: _hip.heston_scenarios(scenarios, N, M, SEED, anti, off))


@pytest.mark.parametrize("scheme", ["euler", "qe"])
def test_heston_autocallable_and_cliquet(scheme):
    is_qe = scheme == "qe"
    model = qe.STEEP if is_qe else HESTON
    sweep("heston_autocallable " + scheme,
          lambda N, M, anti, off: _hip.heston_autocallable(S, T, R, Q, *model, *AUTOCALL, OBSERVATION_FREQ[M], N, M, SEED, anti, off, qe=is_qe))
    sweep("heston_cliquet " + scheme,
          lambda N, M, anti, off: _hip.heston_cliquet(S, T, R, Q, *model, *CLIQUET, PERIODS[M], N, M, SEED, anti, off, qe=is_qe))


@pytest.mark.parametrize("degree", [1, 4])
def test_american_lsm(degree):
    """The path launch strides and, with the cap below the CU count, so do the step kernels."""
    want = memo(lambda N, M: po.american_lsm(S, 100.0, T, R, SIG, Q, False, N, M, degree, SEED))
    sweep("american_lsm", lambda N, M, anti, off: _hip.american_lsm(S, 100.0, T, R, SIG, Q, False, N, M, degree, SEED),
          lambda st, N, M, anti, off, label: check_two("american_lsm", st, want(N, M), 1, max(S, 100.0), label),
          offsets=(0,), antithetic=(False,))


# ------------------------------------------------------------------------------------------------------ per-path outputs ----
def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def per_path(entry, call, steps=STEPS):
    for N in PATHS:
        for M in steps:
            plain = call(N, M)
            for cap in CAPS:
                with grid_cap(cap):
                    capped = call(N, M)
                assert len(capped) == len(plain)
                for a, b in zip(capped, plain):
                    assert np.isfinite(b).all() and same_bytes(a, b), (entry, N, M, cap)


@pytest.mark.parametrize("anti", [False, True])
def test_terminal_prices_are_the_same_bytes(anti):
    per_path("european_terminal", lambda N, M: [_hip.european_terminal(S, T, R, SIG, Q, N, M, SEED, anti)], steps=(5, 67, 252, 257))


@pytest.mark.parametrize("path_major", [False, True])
def test_path_matrices_are_the_same_bytes(path_major):
    per_path("gbm_paths", lambda N, M: [_hip.gbm_paths(S, T, R, SIG, Q, N, M, SEED, path_major)])
    per_path("heston_paths", lambda N, M: _hip.heston_paths(S, T, R, Q, *HESTON, N, M, SEED, path_major))
    per_path("heston_qe_paths", lambda N, M: _hip.heston_qe_paths(S, T, R, Q, *qe.STEEP, N, M, SEED, path_major))
    for model in (MERTON, KOU):
        per_path("jump_paths", lambda N, M: [_hip.jump_paths(S, T, R, SIG, Q, *model, N, M, SEED, path_major)])


# ---------------------------------------------------------------------------------- fused launches that keep their grid ----
def greeks_bits(result):
    out9, evals = result
    return [float(x).hex() for x in out9] + [(e.n, float(e.sum).hex(), float(e.sumsq).hex()) for e in evals]


def test_fused_entry_points_keep_their_grid_and_their_bits():
    N, M = 769, 67
    sv, shift = sobol_tables(M, 7, N)
    opts = [(S + i, K, T, R, SIG + 0.01 * (i % 3), Q, bool(i % 2)) for i in range(14)]
    calls = {
        "european_greeks_fd": lambda: greeks_bits(_hip.european_greeks_fd(S, K, T, R, SIG, Q, True, N, M, SEED, True)),
        "asian_greeks_fd": lambda: greeks_bits(_hip.asian_greeks_fd(S, K, T, R, SIG, Q, True, N, M, SEED, True, True)),
        "extrema_greeks_fd": lambda: greeks_bits(_hip.extrema_greeks_fd(S, K, T, R, SIG, Q, True, 0, 125.0, N, M, SEED, True, True)),
        "european_qmc_batch": lambda: [(e.n, float(e.sum).hex(), float(e.sumsq).hex()) for e in _hip.european_qmc_batch(opts, N, sv, shift)],
        "european_qmc_greeks_fd": lambda: greeks_bits(_hip.european_qmc_greeks_fd(S, K, T, R, SIG, Q, True, N, sv, shift, True)),
    }
    for entry, call in calls.items():
        plain = call()
        with grid_cap(1):
            assert call() == plain, entry


# =============================================================================================================== Sobol ====
@pytest.mark.parametrize("n", [13, 130, 252])
def test_sobol_asian_barrier_and_lookback(n):
    """A wave per point, 125 trips; the bridge at n = 130 fills its LDS row in three trips and the next point reuses the row."""
    with grid_cap(SOBOL_CAP):
        for i, (cls, first) in enumerate(SOBOL_FIRSTS):
            hi.check_exotics(n, "cap 2, first " + cls, first, SOBOL_POINTS, (7, 1234)[i], hi.EXOTIC_KINDS)


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_sobol_fused_path_greeks(construction):
    """qmc_path_greeks_kernel strides like the one-contract kernel (its launch takes the same capped grid): every evaluation of
    asian_qmc_greeks_fd / extrema_qmc_greeks_fd against its own launch -- which the test above ties to the oracle -- at
    tests/test_gpu_exotic_qmc_greeks.py's bar, 130 dates, 8 and 14 contracts."""
    with grid_cap(SOBOL_CAP):
        xg._check_evaluations(130, construction, SOBOL_POINTS, 29, [(True, True), (False, False)])


@pytest.mark.parametrize("n", [50, 252])
def test_sobol_autocallable_and_cliquet(n):
    with grid_cap(SOBOL_CAP):
        for i, (cls, first) in enumerate(SOBOL_FIRSTS):
            hi.check_structured(n, "cap 2, first " + cls, first, SOBOL_POINTS, (7, 1234)[i])


@pytest.mark.parametrize("n", [13, 130])
def test_sobol_heston_and_its_path_payoffs(n):
    """Lanes over points: 16 blocks on 8 waves, the second trip ragged (first = 0) or ragged at both ends; every wave's bridge slab
    (2 n doubles per lane) is reused."""
    with grid_cap(SOBOL_CAP):
        for i, (cls, first) in enumerate(SOBOL_FIRSTS):
            for model in hq.MODELS[:2]:
                hi.check_heston(n, "cap 2, first " + cls, first, SOBOL_POINTS, (7, 1234)[i], model, hi.HESTON_FAMILIES)


def test_sobol_heston_surface_euler():
    """tests/test_gpu_heston_surface.py's oracle and bar: bridge and sequential, both legs, calls and puts, 13 steps."""
    with grid_cap(SOBOL_CAP):
        hsf.test_sobol_cells_match_the_numpy_oracle(13, 0, SOBOL_POINTS)


def test_sobol_heston_surface_qe():
    """tests/test_gpu_heston_qe.py's restatement on SciPy's points, at its TIE on the cells' sums."""
    n, seed, model = 16, 5, qe.STEEP
    draws = hqe.sobol_draws(n, SOBOL_POINTS, seed)
    legs = []
    for mirror in (False, True):
        spot, _var, _quadratic, psi = qe.paths(hqe.S, model, hqe.R, hqe.Q, hqe.T, n, *draws, mirror=mirror)
        assert not np.any(np.abs(psi - qe.PSI_C) < 1e-9)                            # the sums need every path on the branch the oracle took
        legs.append(spot)
    cells = surface_cells(n)
    sv, shift = sobol_tables(2 * n, seed, SOBOL_POINTS)
    for option_type in ("call", "put"):
        for antithetic in (False, True):
            with grid_cap(SOBOL_CAP):
                stats = _hip.heston_qe_qmc_surface(hqe.S, hqe.T, hqe.R, hqe.Q, option_type == "call", *model, [k for k, _ in cells],
                                                   [m for _, m in cells], SOBOL_POINTS, sv, shift, False, antithetic)
            for st, (strike, step) in zip(stats, cells):
                x = np.concatenate([hqe.payoff(spot, strike, step, option_type) for spot in (legs if antithetic else legs[:1])])
                record("heston_qe_qmc_surface", "capped vs oracle, relative", abs(st.sum - float(np.sum(x))) / max(float(np.sum(x)), 1e-300))
                assert st.n == len(x)
                assert st.sum == pytest.approx(float(np.sum(x)), **hqe.TIE), (option_type, antithetic, strike, step)
                assert st.sumsq == pytest.approx(float(np.sum(x * x)), **hqe.TIE), (option_type, antithetic, strike, step)


def test_sobol_heston_scenarios():
    """tests/test_gpu_heston_scenarios.py's oracle and bar: the MIXED and GREEKS sets, both constructions, both legs, 13 steps."""
    with grid_cap(SOBOL_CAP):
        hsc.test_sobol_scenarios_match_the_numpy_oracle(13, 0, SOBOL_POINTS)


def test_sobol_heston_products_euler():
    with grid_cap(SOBOL_CAP):
        hst.check_euler_sobol(13, 4, 4, SOBOL_POINTS, hpo.USUAL, 3, ("bridge", "sequential"))


def test_sobol_heston_products_qe():
    n, f, periods, seed, model = 13, 4, 4, 5, qe.STEEP
    label = ("qe sobol, cap 2", n, f, periods, SOBOL_POINTS, seed)
    legs = hst.qe_legs(model, n, qe.sobol_draws(n, SOBOL_POINTS, seed), label)
    with grid_cap(SOBOL_CAP):
        plain = (hst.sobol_autocall(model, f, SOBOL_POINTS, n, seed, "sequential", True), hst.sobol_cliquet(model, periods, SOBOL_POINTS, n, seed, "sequential", True))
        both = (hst.sobol_autocall(model, f, SOBOL_POINTS, n, seed, "sequential", True, antithetic=True),
                hst.sobol_cliquet(model, periods, SOBOL_POINTS, n, seed, "sequential", True, antithetic=True))
    hst.check_both_products(label, legs[:1], f, periods, *plain)
    hst.check_both_products(label, legs, f, periods, *both)


@pytest.mark.parametrize("construction", ["bridge", "sequential"])
def test_sobol_path_matrices_and_the_american_option(construction):
    """1000 points x 13 dates from point 0 (these calls take no offset): lsm_qmc_paths_kernel, heston_qmc_paths_kernel and the QE
    matrix kernel take two trips; the American chain reads the capped matrix."""
    n, count, seed, bridge = 13, SOBOL_POINTS, 7, construction == "bridge"
    Sa, sigma, q, Ka = 100.0, 0.25, 0.01, 100.0
    sv, shift = hi.tables(n, seed)
    want = sr.gbm_prices(sr.point_normals(sv, shift, 0, count), bridge, Sa, am.T, am.R, sigma, q)
    with grid_cap(SOBOL_CAP):
        pm = _hip.gbm_qmc_paths(Sa, am.T, am.R, sigma, q, count, sv, shift, bridge, path_major=True)
        tm = _hip.gbm_qmc_paths(Sa, am.T, am.R, sigma, q, count, sv, shift, bridge, path_major=False)
        st = _hip.american_lsm_qmc(Sa, Ka, am.T, am.R, sigma, q, False, count, sv, shift, bridge, 3)
    hi.record("gbm_qmc_paths", "cap 2", pm, want)
    assert pm.shape == (count, n + 1) and np.array_equal(pm, tm.T)
    assert np.allclose(pm, want, rtol=1e-11, atol=0)
    pm[:, 0] = am.reference_column0(Sa, count)
    price, x = orc.american_from_paths(pm, Ka, am.T, am.R, "put", 3, return_payoffs=True)
    hi.record("american_lsm_qmc", "cap 2", [st.sum, st.price], [np.sum(x), price])
    am.assert_tied(st, price, x, am.AMERICAN_TIE)
    # Heston: spot and variance, both layouts
    sv2, shift2 = hi.tables(2 * n, seed)
    spot_o, var_o = hq.literal_recursion(*hq.step_normals(sr.point_normals(sv2, shift2, 0, count), construction), hq.USUAL, n)
    with grid_cap(SOBOL_CAP):
        spot, var = _hip.heston_qmc_paths(hq.S, hq.T, hq.R, hq.Q, *hq.USUAL, count, sv2, shift2, bridge, path_major=True)
        spot_t, var_t = _hip.heston_qmc_paths(hq.S, hq.T, hq.R, hq.Q, *hq.USUAL, count, sv2, shift2, bridge, path_major=False)
    hi.record("heston_qmc_paths", "cap 2", spot, spot_o)
    assert np.array_equal(spot_t.T, spot) and np.array_equal(var_t.T, var)
    assert np.allclose(spot, spot_o, rtol=1e-11, atol=0)
    assert np.allclose(var, var_o, rtol=1e-11, atol=1e-11 * hq.USUAL[4])              # test_a_long_heston_path_matrix's bar, and why
    if not bridge:                                                                    # QE takes the sequential construction only
        with grid_cap(SOBOL_CAP):
            q_spot, q_var = _hip.heston_qe_qmc_paths(hqe.S, hqe.T, hqe.R, hqe.Q, *qe.STEEP, count, sv2, shift2, path_major=True)
            t_spot, t_var = _hip.heston_qe_qmc_paths(hqe.S, hqe.T, hqe.R, hqe.Q, *qe.STEEP, count, sv2, shift2, path_major=False)
        assert np.array_equal(q_spot, t_spot.T) and np.array_equal(q_var, t_var.T)
        hqe.check_paths(("sobol, cap 2", count, n, "steep", seed), qe.STEEP, q_spot, q_var,
                        qe.paths(hqe.S, qe.STEEP, hqe.R, hqe.Q, hqe.T, n, *qe.sobol_draws(n, count, seed)))
