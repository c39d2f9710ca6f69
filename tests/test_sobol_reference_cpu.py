"""CPU checks of tests/sobol_reference.py: the plain restatement of the scrambled-Sobol points against SciPy's own engine, the two
table routes of optionslab_amd.monte_carlo.sobol_tables against the same points, index_where's round trip, and every path oracle that
took a z= parameter against what it computed from point 0 before."""
import time
import warnings

import numpy as np
import pytest
from scipy.special import ndtri
from scipy.stats import qmc

from optionslab_amd import monte_carlo as mc
from tests import sobol_reference as sr

SEEDS = (7, 1234, 2**31 - 5)
TOP = (1 << 30) - 1


def engine_tables(d, seed):
    eng = qmc.Sobol(d=d, scramble=True, seed=seed)
    return eng, np.asarray(eng._sv, dtype=np.uint64), np.asarray(eng._shift, dtype=np.uint64)


def draw(eng, n):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return eng.random(n)


@pytest.mark.parametrize("d", [1, 3, 252])
@pytest.mark.parametrize("seed", SEEDS)
def test_points_are_scipys_from_point_0(d, seed):
    eng, sv, shift = engine_tables(d, seed)
    x = sr.points(sv, shift, np.arange(4096))
    assert x.dtype == np.uint64 and x.shape == (4096, d)
    assert np.array_equal(x.astype(np.float64), draw(eng, 4096) * 2.0**30)
    assert np.array_equal(sr.uniforms(x), draw(qmc.Sobol(d=d, scramble=True, seed=seed), 4096))


@pytest.mark.parametrize("d,off", [(252, 1 << 20), (2, (1 << 26) + 4321), (1, (1 << 29) + (1 << 27) + 5)])
def test_points_are_scipys_far_into_the_sequence(d, off):
    """fast_forward is linear in off x d; the last case sets bits 27..29 of the index."""
    eng, sv, shift = engine_tables(d, 13)
    t0 = time.perf_counter()
    eng.fast_forward(off)
    print(f"fast_forward(d={d}, {off}) took {time.perf_counter() - t0:.2f} s")
    want = draw(eng, 1000)
    x = sr.points(sv, shift, off + np.arange(1000))
    assert np.array_equal(x.astype(np.float64), want * 2.0**30)


@pytest.mark.parametrize("d,seed,derived_bits", [(1, 7, 30), (64, 1234, 20)])
def test_both_table_routes_give_the_same_points(d, seed, derived_bits):
    """sobol_tables(d, seed, 2^30) -- the private _sv / _shift route -- and the route derived from the engine's public behaviour.
    Deriving costs a fast_forward over the whole range per table (linear in 2^bits x d): all 30 columns for one dimension, 20 columns
    for 64 dimensions, compared on the points those columns select."""
    mc._sobol_cache.clear()
    sv, shift = mc.sobol_tables(d, seed, 1 << 30)
    mc._sobol_cache.clear()
    dsv, dshift = mc._derive_sobol_tables(qmc.Sobol, d, seed, derived_bits)
    _eng, esv, eshift = engine_tables(d, seed)
    assert getattr(sv, "valid_bits", 30) == 30
    assert np.array_equal(np.asarray(sv), esv) and np.array_equal(shift, eshift)
    ks = np.concatenate([np.arange(100), (1 << 29) + np.arange(100), (1 << 30) - 100 + np.arange(100), [0x2AAAAAAA, 0x15555555]])
    want = sr.points(esv, eshift, ks)
    assert np.array_equal(sr.points(sv, shift, ks), want)
    assert np.array_equal(mc.expand_sobol_points(np.asarray(sv), shift, (1 << 30) - 5, 5), sr.uniforms(want[295:300]))
    assert not dsv[:, derived_bits:].any()
    ks = ks & ((1 << derived_bits) - 1)
    assert np.array_equal(sr.points(dsv, dshift, ks), sr.points(esv, eshift, ks))


@pytest.mark.parametrize("d,seed", [(64, 7), (252, 1234), (8, 5)])
def test_index_where_round_trips(d, seed):
    _eng, sv, shift = engine_tables(d, seed)
    for t in (0, d // 2, d - 1):
        for target in (0, TOP, 0x12345678):
            k = sr.index_where(sv[t], shift[t], target)
            assert k is not None and 0 <= k < (1 << 30), (d, seed, t, target)
            x = sr.points(sv, shift, [k])
            assert int(x[0, t]) == target
            z = sr.normals(x)[0, t]
            if target == 0:
                assert z == ndtri(1e-10) and z == pytest.approx(-6.3613, abs=1e-4)        # the clip
            elif target == TOP:
                assert z == ndtri(1 - 2.0**-30) and z < -ndtri(1e-10)                     # below 1 - 1e-10: no clip
    assert sr.index_where([1 << b for b in range(30)], 0, 0b1000) == 0b1111               # identity directions: k = gray^-1(target)
    dependent = [1 << b for b in range(29)] + [3]
    assert sr.index_where(dependent, 0, 5) is None


def test_the_restated_normals_are_the_reference_pipelines():
    """norm.ppf(np.clip(u, 1e-10, 1 - 1e-10)) of gbm_qmc.py:36 and ndtri of the same argument are the same numbers."""
    from scipy.stats import norm

    eng, sv, shift = engine_tables(5, 99)
    u = draw(eng, 2048)
    assert np.array_equal(sr.normals(sr.points(sv, shift, np.arange(2048))), norm.ppf(np.clip(u, 1e-10, 1 - 1e-10)))
    assert np.array_equal(sr.point_normals(sv, shift, 100, 50), norm.ppf(np.clip(u[100:150], 1e-10, 1 - 1e-10)))


# ------------------------------------------------------------------------- the oracles that took z= equal their old selves ----
def _z(d, seed, n_points):
    _eng, sv, shift = engine_tables(d, seed)
    return sr.point_normals(sv, shift, 0, n_points)


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        va, vb = a[key], b[key]
        if isinstance(va, tuple):
            assert all(np.array_equal(x, y) for x, y in zip(va, vb)), key
        else:
            assert np.array_equal(va, vb), key


@pytest.mark.parametrize("n,N", [(1, 100), (3, 2500), (50, 3000)])
def test_the_exotic_oracle_on_given_normals_equals_itself_from_point_0(n, N):
    from tests import test_gpu_exotic_qmc as ex

    for bridge in (True, False):
        for mirror in (False, True):
            _same(ex.oracle_payoffs(n, N, 7, bridge, mirror), ex.oracle_payoffs(n, N, 7, bridge, mirror, z=_z(n, 7, N)))


@pytest.mark.parametrize("n,N", [(3, 2500), (50, 3000)])
def test_the_structured_oracle_on_given_normals_equals_itself_from_point_0(n, N):
    from tests import test_gpu_structured_qmc as stq

    jobs = [(stq.auto_payoffs, 2, {}), (stq.cliq_payoffs, 3, {})]
    _same(stq.oracle_vectors(n, N, 1234, jobs), stq.oracle_vectors(n, N, 1234, jobs, z=_z(n, 1234, N)))
    # and the shared price matrix is the one this oracle builds
    mine = sr.gbm_prices(_z(n, 1234, N), False, stq.S, stq.T, stq.R, stq.SIG, stq.Q)
    theirs = np.concatenate([c[("sequential", 0)] for c in stq.oracle_paths(n, N, 1234)])
    assert np.array_equal(mine, theirs)


@pytest.mark.parametrize("n,N", [(1, 100), (20, 2500)])
def test_the_heston_oracles_on_given_normals_equal_themselves_from_point_0(n, N):
    from tests import heston_path_oracle as hpo
    from tests import test_gpu_heston_qmc as hq

    z = _z(2 * n, 5, N)
    _same(hq.oracle_paths(n, N, 5, hq.USUAL), hq.oracle_paths(n, N, 5, hq.USUAL, z=z))
    both = ("bridge", "sequential")
    _same(hpo.sobol_spots(n, N, 5, hpo.FELLER_VIOLATING, both), hpo.sobol_spots(n, N, 5, hpo.FELLER_VIOLATING, both, z=z))


def test_the_american_path_oracle_on_given_normals_equals_itself_from_point_0():
    from tests import test_gpu_american_qmc as am

    n, N = 2, 5000
    for bridge in (True, False):
        old = list(am.oracle_paths(100.0, 1.0, 0.05, 0.25, 0.01, n, N, 7, bridge))
        new = list(am.oracle_paths(100.0, 1.0, 0.05, 0.25, 0.01, n, N, 7, bridge, z=_z(n, 7, N)))
        assert [r for r, _ in old] == [r for r, _ in new] == [0, 4096]
        assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(old, new))
