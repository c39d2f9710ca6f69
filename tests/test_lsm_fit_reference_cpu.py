"""CPU checks of tests/lsm_fit_reference.py, the exact reference of the in-wave solvers ha_fit<D> and LsmFit, and of the designs it hands
to tests/test_gpu_lsm_fit.py.  No GPU: the library is loaded for olha_regressor_scales (host arithmetic), never a device.

  index rules   the moment matrix the reference gathers from a row of totals is A^T A of the monomials themselves, entry by entry
  exact solve   on a system with a known answer; the pin rule removes a row and a column and nothing else
  designs       every exact pivot ratio is 0 or outside [1e-12, 1e-10] (asserted, not skipped: a design that fell inside was replaced
                when the reference was written); the singular patterns pin the unknowns the prototype found; the threshold designs
                sit in their bands; no fitted unknown has an exact coefficient of 0 (the GPU test reads `== 0.0` as "pinned")
  restatement   heston_american_oracle.normal_equations_fit, the NumPy restatement of the device's algorithm, agrees with the exact
                reference on pins and `valid` on every design, and its backward error is printed in the units of the GPU test
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import heston_american_oracle as hao
from tests import lsm_fit_reference as ref
from tests.abi_support import library  # noqa: F401  (fixture: the realistic family asks the library for its scales)

IDS = [f"{s}-{d}" for s, d in ref.SOLVERS]


def _design_matrix(solver, degree, points):
    x, y, _cf = points
    return hao.monomials(x, y if solver == "ha" else None, degree)


# --------------------------------------------------------------------------------------------------- the index rules ----
@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_the_gathered_matrix_is_the_gram_matrix_of_the_monomials(library, solver, degree):
    design = ref.designs(solver, degree)[0]
    assert design.family == "generic"
    A = _design_matrix(solver, degree, design.points)                        # dyadic: every product and partial sum below is exact in fp64
    M, b, count = ref.system(solver, degree, design.totals)
    gram, rhs = A.T @ A, A.T @ design.points[2]
    assert [[float(v) for v in row] for row in M] == gram.tolist() and [float(v) for v in b] == rhs.tolist()
    assert count == A.shape[0] == 4000 and len(M) == ref.unknowns(solver, degree) and len(design.totals) == ref.width(solver, degree)
    assert all(M[r][c] == M[c][r] for r in range(len(M)) for c in range(r))


def test_the_index_rule_of_the_two_factor_basis():
    assert [ref.ha_index(a, b) for a, b in ref.ha_monomials(3)] == list(range(10))
    assert ref.ha_monomials(2) == [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]
    assert [ref.ha_sizes(d) for d in (1, 2, 3)] == [(3, 6, 10), (6, 15, 22), (10, 28, 39)]
    assert sorted(ref.ha_index(a, b) for a, b in ref.ha_monomials(6)) == list(range(28))


# --------------------------------------------------------------------------------------------------- the exact solve ----
def test_the_exact_solve_returns_a_known_answer_and_pins_by_removing_a_row_and_a_column():
    # degree-2 one-factor system made from a known beta: M = [[4, 2, 6], [2, 6, 8], [6, 8, 18]] (sum z^m of z = -1, 0, 1, 2), b = M beta
    moments = [4, 2, 6, 8, 18, 32, 66, 128, 258]
    beta = [Fraction(3, 2), Fraction(-2), Fraction(1, 4)]
    totals = [0.0] * ref.LSM_NV
    totals[:9] = moments
    for r in range(3):
        totals[ref.LSM_RHS + r] = float(sum(moments[r + c] * beta[c] for c in range(3)))
    totals[ref.LSM_COUNT] = 4.0
    fit = ref.solve("lsm", 2, totals)
    assert fit.valid and fit.pinned == frozenset() and fit.beta == beta
    assert fit.ratios[0] == 1 and fit.ratios[1] == Fraction(5, 6)            # 6 - 2 * 2 / 4 = 5 of 6
    assert ref.backward_error(fit, [1.5, -2.0, 0.25]) == (0, 64)             # the widest row 6 + 8 + 18 times the largest |beta|, 2
    assert ref.backward_error(fit, [1.5, -2.0, 0.5]) == (Fraction(9, 2), 64)  # the last row's 18 x 1/4
    totals[ref.LSM_COUNT] = 3.0
    assert not ref.solve("lsm", 2, totals).valid and ref.solve("lsm", 2, totals).beta == [0, 0, 0]
    # z = -1, 1 twice each: z^2 = 1, the third pivot is exactly 0; the others are the fit of 1, z
    totals[:9] = [4, 0, 4, 0, 4, 0, 4, 0, 4]
    totals[ref.LSM_RHS:ref.LSM_RHS + 3] = [8.0, 2.0, 8.0]
    totals[ref.LSM_COUNT] = 4.0
    fit = ref.solve("lsm", 2, totals)
    assert fit.pinned == frozenset({2}) and fit.ratios[2] == 0 and fit.beta == [2, Fraction(1, 2), 0]


# ------------------------------------------------------------------------------------------------------- the designs ----
@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_no_pivot_of_any_design_is_near_the_threshold(library, solver, degree):
    families = set()
    for design, fit in zip(ref.designs(solver, degree), ref.fits(solver, degree)):
        families.add(design.family)
        inside = [(k, float(r)) for k, r in enumerate(fit.ratios) if r != 0 and ref.BAND[0] <= r <= ref.BAND[1]]
        assert not inside, (design.family, design.name, inside)
        assert np.all(np.isfinite(design.totals))
        if fit.valid:
            assert all(fit.beta[k] != 0 for k in range(len(fit.beta)) if k not in fit.pinned), (design.family, design.name)
    assert families == {"generic", "realistic", "singular", "gate", "threshold"}


PROTOTYPE_PINS = [("ha", 1, "y = 0", [2]), ("ha", 2, "y = 0", [2, 4, 5]), ("ha", 3, "y = 0", [2, 4, 5, 7, 8, 9]),
                  ("ha", 1, "y = 3/8", [2]), ("ha", 2, "y = x", [2, 4, 5]), ("ha", 3, "y = 2x - 1/4", [2, 4, 5, 7, 8, 9]),
                  ("ha", 2, "x two-valued", [3]), ("ha", 3, "x two-valued", [3, 6, 7]), ("ha", 3, "y three-valued", [9])]


def test_the_singular_patterns_pin_what_the_prototype_found(library):
    named = {(s, d, design.name): fit for s, d in ref.SOLVERS for design, fit in zip(ref.designs(s, d), ref.fits(s, d))}
    for solver, degree, name, pins in PROTOTYPE_PINS:
        assert sorted(named[solver, degree, name].pinned) == pins, (solver, degree, name)
    # and every pattern pins what its design says (x = 0, y two-valued, z on `degree` levels: by the same reasoning)
    seen = 0
    for solver, degree in ref.SOLVERS:
        for design, fit in zip(ref.designs(solver, degree), ref.fits(solver, degree)):
            if design.pinned is not None:
                assert sorted(fit.pinned) == sorted(design.pinned) and fit.valid, (solver, degree, design.name)
                seen += 1
            if design.family == "singular":
                assert all(fit.ratios[k] == 0 for k in fit.pinned), "singular in the totals, bit for bit"
    assert seen >= 3 * 6 + 2 + 1 + 4 + 2 * 7


@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_the_threshold_designs_sit_in_their_bands(library, solver, degree):
    n = ref.unknowns(solver, degree)
    bands = []
    for design, fit in zip(ref.designs(solver, degree), ref.fits(solver, degree)):
        if design.family != "threshold":
            continue
        lo, hi = design.last_ratio_band
        ratio = fit.ratios[design.band_of]
        print(solver, degree, design.name, "ratio", float(ratio), "pinned", sorted(fit.pinned))
        assert lo <= ratio <= hi, (design.name, float(ratio))
        assert ((design.band_of % n) in fit.pinned) == (hi <= ref.PIN)
        bands.append((lo, hi))
    assert ref.FITTED_BAND in bands and ref.PINNED_BAND in bands
    assert ref.FITTED_BAND == (Fraction(1, 10 ** 10), Fraction(1, 10 ** 9)) and ref.PINNED_BAND == (Fraction(1, 10 ** 13), Fraction(1, 10 ** 12))


@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_the_gate_designs_straddle_the_count(library, solver, degree):
    n = ref.unknowns(solver, degree)
    got = {design.name: fit.valid for design, fit in zip(ref.designs(solver, degree), ref.fits(solver, degree)) if design.family == "gate"}
    want = {f"{c} points": c > n for c in (n - 1, n, n + 1, n + 2)}
    want.update({f"count lane {c}": c > n for c in (n - 1, n, n + 1, n + 2)})
    assert got == want


# --------------------------------------------------------------------------------------------------- the restatement ----
@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_the_numpy_restatement_agrees_on_pins_and_valid(library, solver, degree):
    """heston_american_oracle.normal_equations_fit on the points themselves where the design has points, its algorithm on the totals'
    own matrix (lsm_fit_reference.numpy_fit) everywhere.  Its pins are the coefficients it leaves at exactly 0."""
    n = ref.unknowns(solver, degree)
    worst, with_points = 0.0, 0
    for design, fit in zip(ref.designs(solver, degree), ref.fits(solver, degree)):
        beta, pins = ref.numpy_fit(solver, degree, design.totals)
        assert pins == fit.pinned, (design.family, design.name, sorted(pins), sorted(fit.pinned))
        assert (design.totals[ref.width(solver, degree) - 1 if solver == "ha" else ref.LSM_COUNT] > n) == fit.valid
        if fit.valid:
            residual, scale = ref.backward_error(fit, beta)
            assert residual <= ref.ceiling(n) * scale
            worst = max(worst, float(residual / (scale * ref.U)))
        if design.points is not None:
            A = _design_matrix(solver, degree, design.points)
            oracle_beta = hao.normal_equations_fit(A, design.points[2])
            assert frozenset(k for k in range(n) if oracle_beta[k] == 0.0) == fit.pinned, (design.family, design.name)
            assert (A.shape[0] > A.shape[1]) == fit.valid                      # american_from_state's gate
            if design.family != "threshold":                                    # dyadic points: A^T A is the totals' matrix, bit for bit
                assert np.array_equal(oracle_beta, beta), (design.family, design.name)
            with_points += 1
    print(f"{solver} degree {degree}: the NumPy restatement's worst backward error {worst:.3f} u |M| |beta| (ceiling {3 * n ** 3})")
    assert with_points >= 3 + 1 + 4 + 2
