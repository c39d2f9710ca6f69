"""The two in-wave solvers of the LSM chains on the device -- ha_fit<D> (the American option under Heston, 3 / 6 / 10 unknowns in (x, y))
and LsmFit (the one-factor American option, powers of z up to 4) -- against the EXACT solve of the very system they were handed
(tests/lsm_fit_reference.py: fractions.Fraction on the fp64 totals as given), through the taps olmc_ha_fit_probe / olmc_lsm_fit_probe of
the instrumented build, which run what the step kernels' `fit` lambda runs: workgroup_rows_sum over the set's row, the solve in the first
wave, the barrier, the copy out of LDS, read back by a thread of the last wave.

Whole prices cannot see these solvers fail: every tied pricing keeps its exercise margin above a guard and its moment matrix well
conditioned.  Here each set of totals is one of: generic dyadic designs, the moments of Heston paths in the library's standardised
regressors, patterns that are singular in the totals bit for bit (a pivot that becomes zero DURING elimination: y constant but not zero,
y affine in x, x or y on fewer levels than the degree needs), in-the-money counts on either side of the gate, and a last pivot on
either side of the 1e-11 pin threshold.  Per set:

  1. `valid` is the reference's; an invalid set's coefficients are all == 0.0
  2. the unknowns that are == 0.0 are exactly the reference's pinned ones
  3. backward error over the kept rows and columns, in exact rationals from the device's doubles:
         || M beta - b ||_inf  <=  3 n^3 u || M ||_inf || beta ||_inf,      n unknowns, u = 2^-53
     the elimination bound of a symmetric positive definite matrix in natural order (gamma_3n on |L||U|, || |L||U| || <= n || M ||, the
     remaining n for the changes of norm): independent of the condition number, so the threshold designs are held to it too.  A ceiling,
     not a measurement -- an index slip in the moment gather leaves a residual of order || M || || beta ||, thirteen orders above it.
  4. a set gives the same bits at every position of a launch, whatever its neighbours, and alone

MEASURED worst backward error, in units of u || M ||_inf || beta ||_inf, over all families (ceiling 3 n^3 in brackets):
                              ha 1 (81)   ha 2 (648)   ha 3 (3000)   lsm 1 (24)   lsm 2 (81)   lsm 3 (192)   lsm 4 (375)
    NumPy restatement (CPU)     0.914        0.298        0.064         0.930        0.454        0.599         0.118
    device (MI355X)             0.914        0.519        0.115         0.930        0.483        0.436         0.107
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import lsm_fit_reference as ref
from tests.gpu_support import device_fixture
from tools.probe import binding as probe

pytestmark = pytest.mark.gpu
_device = device_fixture(probe.hip)

IDS = [f"{s}-{d}" for s, d in ref.SOLVERS]
COPIES = 8                      # of every design in one launch: 8 x 35 .. 40 designs, a few hundred sets


def _tap(solver, degree, totals):
    return (probe.ha_fit_probe if solver == "ha" else probe.lsm_fit_probe)(degree, totals)


@functools.lru_cache(maxsize=None)
def launch(solver, degree):
    """(design index of every set, beta, valid) of ONE launch that holds every design COPIES times: the first copies in design order, the
    others shuffled, so that a design meets other neighbours at other positions."""
    designs = ref.designs(solver, degree)
    rng = np.random.default_rng(1000 + 10 * degree + len(solver))
    order = np.concatenate([np.arange(len(designs))] + [rng.permutation(len(designs)) for _ in range(COPIES - 1)])
    beta, valid = _tap(solver, degree, np.array([designs[i].totals for i in order]))
    return order, beta, valid


@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_valid_and_the_pinned_unknowns_are_the_exact_solve_s(solver, degree):
    order, beta, valid = launch(solver, degree)
    designs, fits, n = ref.designs(solver, degree), ref.fits(solver, degree), ref.unknowns(solver, degree)
    assert np.all(np.isfinite(beta)) and set(valid.tolist()) <= {0, 1}
    for j, i in enumerate(order):
        what = (solver, degree, designs[i].family, designs[i].name, "set", j)
        assert bool(valid[j]) == fits[i].valid, what
        assert np.all(beta[j, n:] == 0.0), what                                 # LsmFit: the unknowns beyond the degree
        zero = frozenset(k for k in range(n) if beta[j, k] == 0.0)
        assert zero == (fits[i].pinned if fits[i].valid else frozenset(range(n))), (what, sorted(zero), sorted(fits[i].pinned))


@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_the_backward_error_is_within_the_elimination_bound(solver, degree):
    order, beta, valid = launch(solver, degree)
    designs, fits, n = ref.designs(solver, degree), ref.fits(solver, degree), ref.unknowns(solver, degree)
    worst, by_family, checked = Fraction(0), {}, 0
    for i, (design, fit) in enumerate(zip(designs, fits)):
        if not fit.valid:
            continue
        for bits in {beta[j, :n].tobytes() for j in np.flatnonzero(order == i)}:      # one distinct set of bits, unless test 4 fails
            residual, scale = ref.backward_error(fit, np.frombuffer(bits, dtype=np.float64))
            figure = residual / (scale * ref.U) if scale else Fraction(0)
            by_family[design.family] = max(by_family.get(design.family, Fraction(0)), figure)
            worst = max(worst, figure)
            checked += 1
            assert residual <= ref.ceiling(n) * scale, (solver, degree, design.family, design.name, float(figure), 3 * n ** 3)
    print(f"{solver} degree {degree}: worst backward error {float(worst):.3f} u |M| |beta| over {checked} sets (ceiling {3 * n ** 3}); by family",
          {k: round(float(v), 3) for k, v in by_family.items()})
    assert checked >= len(designs) - 4                                          # all but the gate's four invalid ones


@pytest.mark.parametrize("solver,degree", ref.SOLVERS, ids=IDS)
def test_a_set_gives_the_same_bits_at_every_position_and_alone(solver, degree):
    order, beta, valid = launch(solver, degree)
    designs = ref.designs(solver, degree)
    for i in range(len(designs)):
        at = np.flatnonzero(order == i)
        assert len(at) == COPIES
        assert len({beta[j].tobytes() + valid[j].tobytes() for j in at}) == 1, (solver, degree, designs[i].family, designs[i].name, at.tolist())
    # alone in a launch of one workgroup, and in reverse order: nothing of a launch's other sets reaches a set
    first = {i: int(np.flatnonzero(order == i)[0]) for i in range(len(designs))}
    back_beta, back_valid = _tap(solver, degree, np.array([d.totals for d in reversed(designs)]))
    for i, d in enumerate(designs):
        k = len(designs) - 1 - i
        assert back_beta[k].tobytes() == beta[first[i]].tobytes() and back_valid[k] == valid[first[i]], (solver, degree, d.family, d.name)
    for i in sorted({0, len(designs) // 2, len(designs) - 1}):
        one_beta, one_valid = _tap(solver, degree, designs[i].totals[None, :])
        assert one_beta[0].tobytes() == beta[first[i]].tobytes() and one_valid[0] == valid[first[i]], (solver, degree, designs[i].name)
