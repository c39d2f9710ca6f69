"""tests/path_draw_oracle.py without a device: the tap replaced by tests/box_muller_reference.py.

1. On given normals the oracle is heston_path_oracle.literal_recursion and numpy_reference.full_paths' cumulative sum, to 1e-14.
2. On the oracle's words it is the checker (oracle/philox_gbm.c: gbm_paths, heston_paths, jump_paths) within the checker's own bars, 2e-6
   and 8e-6 with 2e-7 on the variance: the mapping of words to steps and tags is the checker's.
3. The conditions on the Poisson uniforms of every case of tests/test_gpu_path_matrices_exact.py: the inversion loop counts what SciPy's
   quantile counts, no uniform lies within 1e-12 of a step of the CDF (such a path would have to be set aside: none is), and no count
   reaches the cap of 64.
4. The reference's own rounding is not what the GPU module measures: the fp64 and the long-double evaluation differ by less than a
   tenth of TIE (Heston, jump); for GBM, whose bound is one on fp64 rounding itself, the long double is within a tenth of the bound of
   50-digit decimal arithmetic.
"""
import numpy as np
import pytest

from oracle import philox_oracle as po
from tests import heston_path_oracle as hpo
from tests import path_draw_oracle as pdo

S, T, R, Q, SIGMA = pdo.S, pdo.T, pdo.R, pdo.Q, pdo.SIGMA
TAP = pdo.reference_box_muller
REL = 2e-6                                                  # the checker's bar (tests/test_gpu_parity.py); 4 REL on Heston and jump paths
NS = (1, 63, 257, 4133)


def test_long_double_is_wider_here_or_the_oracle_says_so():
    print("np.longdouble mantissa bits", np.finfo(np.longdouble).nmant, "wide", pdo.WIDE)
    assert pdo.LONG is (np.longdouble if pdo.WIDE else np.float64)
    assert float(pdo.z_scale()) == 1.1774100225154747 == float(pdo.z_scale(np.float64))       # kZScale of olmc_host_math.h


# ------------------------------------------------------------------------------- 1. the recursions on given normals ----
def test_gbm_is_the_cumulative_sum_of_full_paths():
    """numpy_reference.full_paths (gbm_numpy.py:86-118) with its normals handed in: log S + cumsum(drift + vol Z)."""
    rng = np.random.default_rng(1)
    for sigma, t_end, r, q in pdo.GBM_PARAMS:
        for n in (1, 4, 13, 64):
            z = rng.standard_normal((257, n))
            dt = t_end / n
            want = np.exp(np.log(S) + np.cumsum((r - q - 0.5 * sigma * sigma) * dt + sigma * np.sqrt(dt) * z, axis=1))
            for dtype in (np.float64, pdo.LONG):
                got = pdo.gbm_paths(S, t_end, r, sigma, q, n, z / float(pdo.z_scale()), dtype)
                assert got.dtype == dtype and np.all(got[:, 0] == S)
                assert np.max(np.abs(got[:, 1:].astype(np.float64) / want - 1.0)) <= 1e-14


@pytest.mark.parametrize("name", sorted(pdo.HESTON_MODELS))
def test_heston_is_the_literal_recursion(name):
    model = pdo.HESTON_MODELS[name]
    rng = np.random.default_rng(2)
    for n in (1, 2, 7, 13):
        z1, z2 = rng.standard_normal((257, n)), rng.standard_normal((257, n))
        for sign, mirror in ((1.0, False), (-1.0, True)):
            want_spot, want_var = hpo.literal_recursion(sign * z1, sign * z2, model, n)
            for dtype in (np.float64, pdo.LONG):
                spot, var = pdo.heston_paths(S, model, T, R, Q, n, z1 / float(pdo.z_scale()), z2 / float(pdo.z_scale()), mirror, dtype)
                assert np.all(spot[:, 0] == S) and np.all(var[:, 0] == model[4]) and np.all(var[:, 1:] >= 0)
                assert np.max(np.abs(spot.astype(np.float64) / want_spot - 1.0)) <= 1e-14
                # a step's variance is a sum of terms up to kappa dt (theta + v) = O(1) at dt = 1 whatever it comes to: what differs is
                # literal_recursion's fp64 rounding of those terms, so the variance is held relative to max(|v|, 1)
                assert np.max(np.abs(var.astype(np.float64) - want_var) / np.maximum(np.abs(want_var), 1.0)) <= 1e-14
    if name == "v0_negative":
        assert np.all(var[:, 1] == var[0, 1]) and np.all(spot[:, 1] == spot[0, 1])                 # the first step is deterministic


# --------------------------------------------------------------------------------- 2. the checker on the same words ----
@pytest.mark.parametrize("seed", (pdo.BIG_SEED, pdo.SMALL_SEED))
def test_gbm_is_the_checker_within_its_bar(seed):
    for sigma, t_end, r, q in pdo.GBM_PARAMS:
        for N, n in ((257, 13), (63, 7), (5, 1), (3, 64)):
            got = pdo.gbm_paths(S, t_end, r, sigma, q, n, pdo.gbm_draws(seed, 0, N, n, TAP))
            want = po.gbm_paths(S, t_end, r, sigma, q, N, n, seed).T
            assert np.allclose(got[:, 1:].astype(np.float64), want[:, 1:], rtol=REL, atol=0), (sigma, N, n)


@pytest.mark.parametrize("name", sorted(pdo.HESTON_MODELS))
def test_heston_is_the_checker_within_its_bar(name):
    model = pdo.HESTON_MODELS[name]
    for seed, N, n in ((pdo.BIG_SEED, 257, 13), (pdo.SMALL_SEED, 63, 7), (pdo.BIG_SEED, 5, 1), (pdo.SMALL_SEED, 5, 2)):
        spot, var = pdo.heston_paths(S, model, T, R, Q, n, *pdo.heston_draws(seed, 0, N, n, TAP))
        want_spot, want_var = po.heston_paths(S, T, R, Q, *model, N, n, seed)
        assert np.allclose(spot.astype(np.float64), want_spot.T, rtol=4 * REL, atol=0), (name, N, n)
        assert np.allclose(var.astype(np.float64), want_var.T, rtol=4 * REL, atol=2e-7), (name, N, n)


@pytest.mark.parametrize("name,model,n", [("M0", pdo.M0, 13), ("M1", pdo.M1, 7), ("K0", pdo.K0, 13), ("K1", pdo.K1, 3), ("K1", pdo.K1, 13),
                                          ("no_jumps", pdo.NO_JUMPS, 5), ("merton_20", pdo.merton_20(2), 2)])
def test_jump_is_the_checker_within_its_bar(name, model, n):
    for seed, N in ((pdo.BIG_SEED, 257), (pdo.SMALL_SEED, 63)):
        got = pdo.jump_oracle(S, T, R, SIGMA, Q, model, n, seed, 0, N, TAP)
        want = po.jump_paths(S, T, R, SIGMA, Q, *model, N, n, seed).T
        assert np.allclose(got["plain"].astype(np.float64), want, rtol=4 * REL, atol=0), (name, N, n)
        if model[1] >= 40.0:
            assert got["counts"].max() >= 2                                                       # steps of several jumps
        # the mirror leg: the same jumps, the diffusion negated
        c = pdo.jump_constants(S, T, R, SIGMA, Q, model, n)
        both = np.log(got["plain"][:, 1:]) + np.log(got["mirror"][:, 1:])
        want_both = 2.0 * (c["log_s0"] + np.cumsum(c["drift"] + got["sums"], axis=1))
        assert np.max(np.abs((both - want_both).astype(np.float64))) <= 1e-13


# --------------------------------------------------------------------- 3. the Poisson uniforms of the GPU module's cases ----
def test_lambda_dt_is_20_exactly_where_the_cases_say_so():
    assert 60.0 * (T / 3) == 20.0 and not pdo.refused(pdo.K1, 3) and pdo.refused(pdo.K1, 2) and pdo.refused(pdo.M1, 1)
    for N in NS:
        for name, model, _seed, n in pdo.jump_cases(N):
            assert not pdo.refused(model, n)
            if name == "merton_20":
                assert model[1] * (T / n) == 20.0
    from scipy.stats import poisson

    assert poisson.ppf(1.0 - 2.0**-33, 20.0) == 54                                  # the largest uniform there is, at the largest rate


@pytest.mark.parametrize("N", NS)
def test_the_loop_counts_what_scipy_counts_and_no_uniform_sits_on_a_step_of_the_cdf(N):
    """Every Poisson uniform of every jump case of the GPU module, and of its launches beyond 2^32."""
    cases = [(model, seed, 0, N, n) for _name, model, seed, n in pdo.jump_cases(N)]
    if N == 1:
        cases += [(model, pdo.BIG_SEED, offset, 1, n) for model in (pdo.M0, pdo.M1, pdo.K0, pdo.K1) for offset in pdo.OFFSETS
                  for n in pdo.OFFSET_STEPS if not pdo.refused(model, n)]
    closest, largest, seen = 1.0, 0, 0
    for model, seed, offset, count, n in cases:
        c = pdo.jump_constants(S, T, R, SIGMA, Q, model, n)
        u = pdo.poisson_uniforms(seed, offset, count, n)
        loop = pdo.counts_by_the_loop(u, c["p0"], c["lam_dt"])
        assert np.array_equal(loop, pdo.counts_by_the_loop(u, c["p0"], c["lam_dt"], np.float64))
        assert np.array_equal(loop, pdo.counts_by_ppf(u, c["lam_dt"])), (model, seed, offset, count, n)
        closest = min(closest, pdo.distance_to_a_cdf_step(u, c["lam_dt"]))
        largest = max(largest, int(loop.max()))
        seen += u.size
    print("uniforms", seen, "closest to a step of the CDF", closest, "largest count", largest)
    assert closest >= 1e-12                                                         # no path is set aside
    assert largest < pdo.JUMP_CAP                                                   # the cap never binds


def test_the_cap_is_where_the_kernel_has_it():
    c = pdo.jump_constants(S, T, R, SIGMA, Q, pdo.merton_20(1), 1)
    cdf = pdo.poisson_cdf_steps(c["p0"], c["lam_dt"])
    assert len(cdf) == 65 and float(cdf[54]) > 1.0 - 2.0**-33 > float(cdf[53])
    assert pdo.counts_by_the_loop(np.array([np.nextafter(1.0, 0.0)]), c["p0"], c["lam_dt"])[0] <= pdo.JUMP_CAP
    assert pdo.counts_by_the_loop(np.array([0.5 * c["p0"], c["p0"]]), c["p0"], c["lam_dt"]).tolist() == [0, 1]


# ------------------------------------------------------------------------------- 4. the reference's own rounding ----
def tie_units(got, want, floor=0.0):
    """|got - want| in units of the project's TIE (rel 1e-10, abs 1e-12), relative to max(|want|, floor)."""
    want = want.astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(1e-10 * np.maximum(np.abs(want), floor), 1e-12)))


def exact_cum(c, z_row):
    """gbm_cum of one path in 50-digit decimal arithmetic: every input is an fp64 value and converts exactly."""
    import decimal

    with decimal.localcontext() as ctx:
        ctx.prec = 50
        scale = (2 * decimal.Decimal(2).ln()).sqrt()
        vol, drift, cum, out = decimal.Decimal(c["vol"]), decimal.Decimal(c["drift"]), decimal.Decimal(0), []
        for z in z_row:
            cum += vol * scale * decimal.Decimal(float(z)) + drift
            out.append(cum)
        return out


def against_exact(cum_row, exact_row):
    """|cum - exact| of one path as fp64, the long double taken apart into two doubles that convert exactly."""
    import decimal

    with decimal.localcontext() as ctx:
        ctx.prec = 50
        hi = cum_row.astype(np.float64)
        lo = (cum_row - hi).astype(np.float64)
        return np.array([float(abs(decimal.Decimal(float(h)) + decimal.Decimal(float(l)) - e)) for h, l, e in zip(hi, lo, exact_row)])


@pytest.mark.skipif(not pdo.WIDE, reason="np.longdouble is fp64 here: the two evaluations are one")
def test_the_gbm_references_own_rounding_is_under_a_tenth_of_the_bound():
    """The GBM bound (t + 8) M 2^-52 is a bound on fp64 rounding itself, so an fp64 evaluation of the oracle -- one rounding of cum per
    step, as on the device -- cannot stay under a tenth of it (measured: 0.2 of the bound at sigma = 1.5), and its distance from the long
    double says nothing about the long double.  So the long-double evaluation is held against 50-digit decimal arithmetic instead: that
    IS the reference's own rounding, and it must be under a tenth of the bound (measured: 1e-4 of it).  The fp64 evaluation is another
    fp64 implementation of the recursion and must meet the whole bound, as the device must."""
    worst_wide, worst_narrow = 0.0, 0.0
    for sigma, t_end, r, q in pdo.GBM_PARAMS:
        for n in (1, 4, 13, 64, 252):
            z = pdo.gbm_draws(pdo.BIG_SEED, 0, 63, n, TAP)
            c = pdo.gbm_constants(S, t_end, r, sigma, q, n)
            wide, narrow = pdo.gbm_cum(c, z), pdo.gbm_cum(c, z, np.float64)
            bound = pdo.gbm_bound(wide)
            worst_narrow = max(worst_narrow, float(np.max(np.abs((narrow - wide).astype(np.float64)) / bound)))
            for i in range(0, 63, 4 if n == 252 else 1):
                worst_wide = max(worst_wide, float(np.max(against_exact(wide[i], exact_cum(c, z[i])) / bound[i])))
    print("in units of the GBM bound: long double against 50 digits", worst_wide, "fp64 against long double", worst_narrow)
    assert worst_wide < 0.1
    assert worst_narrow < 1.0


@pytest.mark.skipif(not pdo.WIDE, reason="np.longdouble is fp64 here: the two evaluations are one")
def test_fp64_and_long_double_differ_by_less_than_a_tenth_of_tie():
    N = 257
    worst = {}
    for name, model in pdo.HESTON_MODELS.items():
        for n in (1, 7, 64):
            z1, z2 = pdo.heston_draws(pdo.BIG_SEED, 0, N, n, TAP)
            for mirror in (False, True):
                narrow, wide = (pdo.heston_paths(S, model, T, R, Q, n, z1, z2, mirror, dtype) for dtype in (np.float64, pdo.LONG))
                worst["heston"] = max(worst.get("heston", 0.0), tie_units(narrow[0], wide[0]), tie_units(narrow[1], wide[1], 1e-2))
    for model, n in ((pdo.M0, 13), (pdo.M1, 7), (pdo.K0, 64), (pdo.K1, 3), (pdo.merton_20(2), 2)):
        narrow, wide = (pdo.jump_oracle(S, T, R, SIGMA, Q, model, n, pdo.BIG_SEED, 0, 63, TAP, dtype) for dtype in (np.float64, pdo.LONG))
        assert np.array_equal(narrow["counts"], wide["counts"])
        worst["jump"] = max(worst.get("jump", 0.0), tie_units(narrow["plain"], wide["plain"]), tie_units(narrow["mirror"], wide["mirror"]))
    print("fp64 against long double, in units of TIE:", worst)
    for family, ratio in worst.items():
        assert ratio < 0.1, (family, ratio)
