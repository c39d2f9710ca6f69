"""The three Philox path matrices against an extended-precision recursion on the stream's own draws (tests/path_draw_oracle.py).

olmc_gbm_paths (lsm_paths_kernel, also behind simulate_gbm_paths_hip), olmc_heston_paths (heston_paths_kernel, Euler) and olmc_jump_paths
/ oljd_paths (jump_paths_kernel, jump_legs_paths_kernel) are the root of the suite's tight ties: the Heston, jump and exotic kernels are
tied at 1e-10 .. 1e-12 to payoffs NumPy computes from these matrices, and the local-volatility paths to normals recovered from the first.
What pinned the matrices themselves was the C checker with libm's fp32 normals, at 2e-6 / 8e-6.  Here the normals are the device's own
(the Philox words from the CPU oracle, passed through the instrumented build's tap of box_muller_raw, bit for bit) and everything after
them is np.longdouble arithmetic on the constants the host folds, so the fp64 part of the kernels is held at fp64's own scale:

  GBM     |ln S_device - ln S_reference| <= (t + 8) M 2^-52 at date t, M = max(1, max |cum|) of the path (path_draw_oracle.gbm_bound
          derives it): 5.8e-14 at t = 252.
  Heston  TIE (rel 1e-10, abs 1e-12) on the spot and on the variance, the variance relative to max(|v|, 1e-2); the reference is the
          LITERAL recursion, the kernel folds its constants, so this bar is not derived.
  jump    TIE on the spot, both entry points, plain and mirror; the counts by the kernel's loop (tests/test_path_draw_oracle_cpu.py
          holds them against SciPy's quantile for these very cases, none set aside).

Every tie prints a line `DEVIATION {json}` before it asserts (pytest -s).  Measured worst values on an MI355X:

  GBM     |ln S_device - ln S_reference| up to 8.3e-15, at most 0.38 of the bound at any state; sigma = 0 against the closed form 0.40 of it.
          Beyond 2^32 (lookback, Asian, plain and antithetic): up to 3.8e-16, at most 0.08 of the bound.
  Heston  spot 7.6e-14 relative (0.0008 of TIE), variance 1.2e-15 absolute (0.0005 of TIE); the exact zeros of the Feller-violating
          model sit at the same states on both sides (6520 of them).  Beyond 2^32 through the surface: 2.9e-15 relative.
  jump    plain 1.3e-14, mirror 1.2e-14 relative (0.00013 of TIE), the sigma = 0 matrix 9e-14; the jump sums read off it within 3.9e-15
          of the oracle's (165,000 jumps, up to 43 in a step).  Beyond 2^32 through the surface: 1.2e-15 relative.

So the Heston and jump kernels sit three to four orders below TIE, and a later change may put derived bars in its place.
"""
import json

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import path_draw_oracle as pdo
from tests.gpu_support import device_fixture, heston_pricer

pytestmark = pytest.mark.gpu

_device = device_fixture()

TIE = dict(rel=1e-10, abs=1e-12)
S, T, R, Q, SIGMA = pdo.S, pdo.T, pdo.R, pdo.Q, pdo.SIGMA
LONG = pdo.LONG
NS = (1, 63, 257, 4133)
WORST = {}                                                  # family -> figure -> the worst seen so far


def TAP(xa, xb):
    from tools.probe import binding as probe

    return probe.box_muller_probe(xa, xb)


def deviation(family, case, **figures):
    """Print the tie's figures and the family's worst so far."""
    worst = WORST.setdefault(family, {})
    for name, value in figures.items():
        worst[name] = max(worst.get(name, 0.0), float(value))
    print("DEVIATION " + json.dumps(dict(family=family, case=[str(c) for c in case], **{k: float(v) for k, v in figures.items()}, worst=worst)))


def rel_dev(got, want):
    return float(np.max(np.abs((got.astype(LONG) / want - 1).astype(np.float64)))) if got.size else 0.0


def tie_units(got, want, floor=0.0):
    """max |got - want| in units of TIE relative to max(|want|, floor): the tie holds where this is <= 1."""
    if got.size == 0:
        return 0.0
    diff = np.abs((got.astype(LONG) - want).astype(np.float64))
    return float(np.max(diff / np.maximum(TIE["rel"] * np.maximum(np.abs(want.astype(np.float64)), floor), TIE["abs"])))


def both_layouts(call):
    """The path-major matrix, after the time-major one has been held equal to it."""
    a, b = call(True), call(False)
    if isinstance(a, tuple):
        for x, y in zip(a, b):
            assert np.array_equal(x, y.T)
    else:
        assert np.array_equal(a, b.T)
    return a


# ------------------------------------------------------------------------------------------------------ the draws ----
def test_the_oracles_words_are_the_devices_words():
    """Integer-exact, every tag the matrices read, also beyond 2^32."""
    for tag, blocks in ((pdo.TAG_GBM, 4), (pdo.TAG_HESTON, 7), (pdo.TAG_JUMP, 7), (pdo.TAG_JUMP_SIZE, 5), (pdo.TAG_JUMP_SIZE + 9, 2)):
        for seed, offset, count in ((pdo.BIG_SEED, 0, 63), (pdo.SMALL_SEED, pdo.OFFSETS[2], 1)):
            assert np.array_equal(_hip.philox_words(seed, offset, count, 0, blocks, tag), pdo.philox_words(seed, offset, count, blocks, tag))


# ------------------------------------------------------------------------------------------------------------ GBM ----
@pytest.mark.parametrize("N", NS)
def test_gbm_paths_are_the_recursion_on_the_devices_draws(N):
    for seed, n in pdo.shapes(N):
        z = pdo.gbm_draws(seed, 0, N, n, TAP)
        for sigma, t_end, r, q in pdo.GBM_PARAMS:
            got = both_layouts(lambda pm: _hip.gbm_paths(S, t_end, r, sigma, q, N, n, seed, path_major=pm))
            assert got.shape == (N, n + 1) and np.all(got[:, 0] == S)
            c = pdo.gbm_constants(S, t_end, r, sigma, q, n)
            cum = pdo.gbm_cum(c, z)
            bound = pdo.gbm_bound(cum)
            log_got = np.log(got[:, 1:].astype(LONG))
            dev = np.abs((log_got - (LONG(c["log_s0"]) + cum)).astype(np.float64))
            figures = dict(log_dev=dev.max(), of_bound=np.max(dev / bound))
            if sigma == 0.0:                                                        # S exp((r - q) t dt), whatever was drawn
                t = np.arange(1, n + 1).astype(LONG)
                want = np.log(LONG(S)) + (LONG(r) - LONG(q)) * t * (LONG(t_end) / LONG(n))
                flat = np.abs((log_got - want).astype(np.float64))
                figures.update(flat_of_bound=np.max(flat / bound))
            deviation("gbm", (N, n, seed, sigma), **figures)
            assert np.all(dev <= bound), (N, n, seed, sigma)
            if sigma == 0.0:
                assert np.all(flat <= bound), (N, n, seed)
    if N == 63:
        assert np.array_equal(ol.simulate_gbm_paths_hip(S, 1.0, 0.01, 0.2, 0.05, N, 13, pdo.SMALL_SEED),
                              _hip.gbm_paths(S, 1.0, 0.01, 0.2, 0.05, N, 13, pdo.SMALL_SEED, path_major=True))


# --------------------------------------------------------------------------------------------------------- Heston ----
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", sorted(pdo.HESTON_MODELS))
def test_heston_euler_paths_are_the_literal_recursion_on_the_devices_draws(name, N):
    model = pdo.HESTON_MODELS[name]
    for seed, n in pdo.shapes(N):
        spot, var = both_layouts(lambda pm: _hip.heston_paths(S, T, R, Q, *model, N, n, seed, path_major=pm))
        assert spot.shape == var.shape == (N, n + 1) and np.all(spot[:, 0] == S) and np.all(var[:, 0] == model[4])
        assert np.all(var[:, 1:] >= 0.0)
        want_spot, want_var = pdo.heston_paths(S, model, T, R, Q, n, *pdo.heston_draws(seed, 0, N, n, TAP))
        zeros_got, zeros_want = var[:, 1:] == 0.0, want_var[:, 1:] == 0.0
        deviation("heston", (name, N, n, seed), spot_rel=rel_dev(spot, want_spot), spot_tie=tie_units(spot, want_spot),
                  var_tie=tie_units(var, want_var, 1e-2), var_abs=np.max(np.abs((var.astype(LONG) - want_var).astype(np.float64))),
                  zeros=int(zeros_want.sum()), zeros_differ=float(np.mean(zeros_got != zeros_want)))
        assert tie_units(spot, want_spot) <= 1.0, (name, N, n, seed)
        assert tie_units(var, want_var, 1e-2) <= 1.0, (name, N, n, seed)
        if name == "feller_violating" and N * n >= 63 * 13:
            assert zeros_got.any() and zeros_want.any()                             # the truncation at 0 binds, on both sides
            assert np.mean(zeros_got != zeros_want) <= 1e-3
        if name == "sigma_v_zero":                                                  # v stays at theta = v0
            assert not zeros_want.any() and not zeros_got.any()
    if N == 63 and name in ("usual", "feller_violating"):                          # the pricer refuses v0 <= 0 and sigma_v = 0: those at the C ABI alone
        a, b = heston_pricer(model).simulate_paths(S, T, R, Q, N, 13, pdo.SMALL_SEED)      # the public method is this matrix
        c, d = _hip.heston_paths(S, T, R, Q, *model, N, 13, pdo.SMALL_SEED, path_major=True)
        assert np.array_equal(a, c) and np.array_equal(b, d)


# ----------------------------------------------------------------------------------------------------------- jump ----
@pytest.mark.parametrize("N", NS)
def test_jump_paths_are_the_recursion_on_the_devices_draws(N):
    for name, model, seed, n in pdo.jump_cases(N):
        label = (name, N, n, seed)
        old = both_layouts(lambda pm: _hip.jump_paths(S, T, R, SIGMA, Q, *model, N, n, seed, path_major=pm))
        plain = both_layouts(lambda pm: _hip.jd_paths(S, T, R, SIGMA, Q, model, N, n, seed, mirror=False, path_major=pm))
        mirror = both_layouts(lambda pm: _hip.jd_paths(S, T, R, SIGMA, Q, model, N, n, seed, mirror=True, path_major=pm))
        assert np.array_equal(old.view(np.uint64), plain.view(np.uint64)), label
        assert old.shape == mirror.shape == (N, n + 1) and np.all(old[:, 0] == S) and np.all(mirror[:, 0] == S)
        want = pdo.jump_oracle(S, T, R, SIGMA, Q, model, n, seed, 0, N, TAP)
        assert int(want["counts"].max()) < pdo.JUMP_CAP
        # the jump sums and where they are, from the device's matrix at sigma = 0: its steps are the compensated drift and the jumps
        flat = _hip.jump_paths(S, T, R, 0.0, Q, *model, N, n, seed, path_major=True)
        c0 = pdo.jump_constants(S, T, R, 0.0, Q, model, n)
        want_flat = pdo.jump_paths(S, T, R, 0.0, Q, model, n, np.zeros((N, n)), want["sums"])
        sums = np.diff(np.log(flat.astype(LONG)), axis=1) - LONG(c0["drift"])
        sums_dev = np.abs((sums - want["sums"]).astype(np.float64))
        deviation("jump", label, plain_rel=rel_dev(old, want["plain"]), plain_tie=tie_units(old, want["plain"]),
                  mirror_rel=rel_dev(mirror, want["mirror"]), mirror_tie=tie_units(mirror, want["mirror"]),
                  flat_tie=tie_units(flat, want_flat), sums_abs=sums_dev.max(), jumps=int(want["counts"].sum()), most=int(want["counts"].max()))
        assert tie_units(old, want["plain"]) <= 1.0, label
        assert tie_units(mirror, want["mirror"]) <= 1.0, label
        assert tie_units(flat, want_flat) <= 1.0, label
        # two spots within rel 1e-10 each: the difference of their logarithms within 2e-10
        assert np.array_equal(np.abs(sums.astype(np.float64)) > 1e-12, want["counts"] > 0), label
        assert np.all(sums_dev <= 2.0 * TIE["rel"]), label
        if name == "no_jumps":
            assert not want["counts"].any()
        if name in ("merton_20", "K1") and model[1] * (T / n) == 20.0:
            assert np.all(want["counts"] > 0) or N * n >= 1000                      # e^-20: a step without a jump is one in 5e8
            assert int(want["counts"].max()) >= 20 or N * n < 4


# ---------------------------------------------------------------------------------------------- paths beyond 2^32 ----
@pytest.mark.parametrize("offset", pdo.OFFSETS)
def test_heston_paths_beyond_2_to_the_32_through_the_surface(offset):
    """The matrices take no offset; a call of strike 0 on one path pays its spot, at every date, and with antithetic = 1 the spot and
    its mirror's."""
    seed = pdo.BIG_SEED
    for name in ("usual", "feller_violating", "v0_negative"):
        model = pdo.HESTON_MODELS[name]
        for n in pdo.OFFSET_STEPS:
            draws = pdo.heston_draws(seed, offset, 1, n, TAP)
            plain = pdo.heston_paths(S, model, T, R, Q, n, *draws)[0][0, 1:]
            mirror = pdo.heston_paths(S, model, T, R, Q, n, *draws, mirror=True)[0][0, 1:]
            dates = list(range(1, n + 1))
            one = _hip.heston_surface(S, T, R, Q, True, *model, [0.0] * n, dates, 1, n, seed, False, offset)
            two = _hip.heston_surface(S, T, R, Q, True, *model, [0.0] * n, dates, 1, n, seed, True, offset)
            got_one, got_two = np.array([st.sum for st in one]), np.array([st.sum for st in two])
            assert all(st.n == 1 for st in one) and all(st.n == 2 for st in two)
            deviation("heston_offset", (name, n, offset), spot_rel=rel_dev(got_one, plain), both_rel=rel_dev(got_two, plain + mirror))
            assert tie_units(got_one, plain) <= 1.0 and tie_units(got_two, plain + mirror) <= 1.0, (name, n, offset)


@pytest.mark.parametrize("offset", pdo.OFFSETS)
def test_jump_paths_beyond_2_to_the_32_through_the_surface(offset):
    seed = pdo.BIG_SEED
    for name, model in (("M0", pdo.M0), ("M1", pdo.M1), ("K0", pdo.K0), ("K1", pdo.K1)):
        for n in pdo.OFFSET_STEPS:
            if pdo.refused(model, n):
                continue
            want = pdo.jump_oracle(S, T, R, SIGMA, Q, model, n, seed, offset, 1, TAP)
            plain, mirror = want["plain"][0, 1:], want["mirror"][0, 1:]
            dates = list(range(1, n + 1))
            one = _hip.jd_surface_prices(S, T, R, SIGMA, Q, True, model, [0.0] * n, dates, 1, n, seed, False, offset)
            two = _hip.jd_surface_prices(S, T, R, SIGMA, Q, True, model, [0.0] * n, dates, 1, n, seed, True, offset)
            got_one, got_two = np.array([st.sum for st in one]), np.array([st.sum for st in two])
            assert all(st.n == 1 for st in one) and all(st.n == 2 for st in two)
            deviation("jump_offset", (name, n, offset), spot_rel=rel_dev(got_one, plain), both_rel=rel_dev(got_two, plain + mirror),
                      jumps=int(want["counts"].sum()))
            assert tie_units(got_one, plain) <= 1.0 and tie_units(got_two, plain + mirror) <= 1.0, (name, n, offset)


@pytest.mark.parametrize("offset", pdo.OFFSETS)
def test_gbm_paths_beyond_2_to_the_32_through_the_lookback_and_the_asian(offset):
    """One path, strike 1: the fixed-strike lookback call pays max_t S_t - 1 over dates 0 .. n, the arithmetic Asian call
    mean_t S_t - 1 over dates 1 .. n; antithetic = 1 adds the mirror's.  Both are positive, so the sum plus the strikes is the maximum
    (the mean), held in the logarithm under the matrix' bound at t = n: the kernels round cum as lsm_paths_kernel does, and the
    roundings that take the place of ln S + cum (S e^x, - 1, the Asian's n additions within its mean) are no more."""
    seed, strike = pdo.BIG_SEED, 1.0
    for sigma, t_end, r, q in pdo.GBM_PARAMS:
        for n in pdo.OFFSET_STEPS:
            z = pdo.gbm_draws(seed, offset, 1, n, TAP)
            c = pdo.gbm_constants(S, t_end, r, sigma, q, n)
            up, down = pdo.gbm_cum(c, z)[0], pdo.gbm_cum(c, -z)[0]
            bound = float(max(pdo.gbm_bound(up[None, :])[0, -1], pdo.gbm_bound(down[None, :])[0, -1]))
            most = [LONG(S) * np.exp(max(LONG(0), leg.max())) for leg in (up, down)]
            mean = [LONG(S) * np.mean(np.exp(leg)) for leg in (up, down)]
            figures = {}
            for label, want, call in (("lookback", most, lambda a: _hip.lookback(S, strike, t_end, r, sigma, q, True, True, 1, n, seed, a, offset)),
                                      ("asian", mean, lambda a: _hip.asian(S, strike, t_end, r, sigma, q, True, False, 1, n, seed, a, offset))):
                one, two = call(False), call(True)
                assert (one.n, two.n) == (1, 2)
                figures[label] = abs(float(np.log((LONG(one.sum) + 1) / want[0])))
                figures[label + "_both"] = abs(float(np.log((LONG(two.sum) + 2) / (want[0] + want[1]))))
            deviation("gbm_offset", (sigma, n, offset), bound=bound, **figures, of_bound=max(figures.values()) / bound)
            assert all(v <= bound for v in figures.values()), (sigma, n, offset, figures, bound)
