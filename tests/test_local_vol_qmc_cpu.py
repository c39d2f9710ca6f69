"""CPU checks of Dupire local volatility on Sobol paths (include/olmc_local_vol_qmc.h, optionslab_amd.DupireLocalVolQMC).

  ABI        olmc_local_vol_qmc.h's declarations = the library's olvq_* exports = _hip.LVQ_PROTOTYPES; the header is C99; the ABI version
             stays 6; every refusal answers OLMC_ERR_ARG with its exact message before any device is touched.
  Python     DupireLocalVolQMC keeps DupireLocalVol's signatures, model.qmc() shares the calibrated surface, the ValueErrors.
  oracle     what tests/test_gpu_local_vol_qmc.py compares the device against: lvo.paths on z (sequential) and on the increments of
             bridge_walk(z) (bridge) equal sobol_reference.gbm_prices on a flat table within 1e-12; for its CASES no path of either leg
             comes within 1e-9 of a barrier level in log space, so the GPU payoff test excludes nothing; the Black-Scholes gap of its
             flat case is below 1e-3.
  scatter    the issue's table at 2^12 x 64: over 16 scrambles against 16 NumPy seeds, the standard deviation of codes 6 and 8 shrinks at
             least 10 x with the bridge and 3 x sequentially (the prototype: 26 / 83 and 7.4 / 5.9).
"""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import local_vol_oracle as lvo
from tests import sobol_reference as sr
from tests import test_gpu_local_vol_qmc as g
from tests.abi_support import assert_header_matches, library, refused
from tests.test_local_vol_cpu import BAD_SURFACES, surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc_local_vol_qmc.h")
NAMES = ["olvq_paths", "olvq_price", "olvq_surface_prices"]

pytestmark = pytest.mark.filterwarnings("ignore:The balance properties of Sobol")


# --------------------------------------------------------------------------------------------------------------- ABI ----
def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "olvq_", _hip.LVQ_PROTOTYPES, NAMES)


def test_header_is_c99(tmp_path):
    from optionslab_amd.build import _hipcc

    cc = shutil.which("gcc") or shutil.which("cc")
    compiler = [cc] if cc else [_hipcc(), "-x", "c"]
    src = tmp_path / "use_header.c"
    src.write_text('#include "olmc_local_vol_qmc.h"\n'
                   "int use(const ollv_surface* s, const uint32_t* sv, const uint32_t* shift, olmc_stats* out) {\n"
                   "    return olvq_price(100, 100, 1, 0.05, 0, 1, s, OLLV_EUROPEAN, 0, OLMC_QMC_BRIDGE, 0, 1000, 8, sv, shift, 30, 0, out); }\n")
    subprocess.run([*compiler, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use_header.o")], check=True)


def entry_calls(library, s, *, payoff=8, barrier=0.0, construction=1, offset=0, n=100, steps=4, k=2, bits=30, out=True, cells=True, matrix=True,
                sv=True, shift=True):
    """The three entry points on the surface pointer s, as thunks that give the return code."""
    st = _hip.Stats()
    sts = (_hip.Stats * 16)()
    strikes, cell_steps = (C.c_double * 16)(*([100.0] * 16)), (C.c_int32 * 16)(*([1] * 16))
    buf = (C.c_double * 8)()
    tables = (C.c_uint32 * 64)()                   # never read: every call here is refused before the tables are
    psv, psh = tables if sv else None, tables if shift else None
    return {
        "olvq_price": lambda: library.olvq_price(100.0, 100.0, 1.0, 0.05, 0.0, 1, s, payoff, barrier, construction, offset, n, steps, psv, psh, bits, 0,
                                                 C.byref(st) if out else None),
        "olvq_paths": lambda: library.olvq_paths(100.0, 1.0, 0.05, 0.0, s, construction, n, steps, psv, psh, bits, 1, buf if matrix else None),
        "olvq_surface_prices": lambda: library.olvq_surface_prices(100.0, 1.0, 0.05, 0.0, 1, s, strikes if cells else None, cell_steps, k, construction,
                                                                   offset, n, steps, psv, psh, bits, 0, sts if out else None),
    }


@pytest.mark.parametrize("entry", NAMES)
def test_every_refusal_answers_its_message_before_any_device_work(library, entry):
    """rc 1 (OLMC_ERR_ARG) and the exact words, on a machine with or without a device: none of these calls initialises one."""
    good, keep = surface()
    call = lambda s=C.byref(good), **kw: entry_calls(library, s, **kw)[entry]()
    # the table, the payoff, the cells and the matrix: ollv_*'s refusals
    refused(library, call(s=None), "null pointer")
    refused(library, call(s=C.byref(_hip.LvSurface(None, 2, 2, -0.5, 0.5, 1.0))), "null pointer")
    refused(library, call(out=False, matrix=False), "null pointer")
    if entry == "olvq_surface_prices":
        refused(library, call(cells=False), "null pointer")
    for kw, message in BAD_SURFACES:
        bad, keep_bad = surface(**kw)
        refused(library, call(s=C.byref(bad)), message)
    if entry == "olvq_price":
        refused(library, call(payoff=-1), "bad payoff")
        refused(library, call(payoff=9), "bad payoff")
        for kind in range(4):
            refused(library, call(payoff=kind, barrier=0.0), "Barrier must be positive")
            refused(library, call(payoff=kind, barrier=-5.0), "Barrier must be positive")
    # the construction, the tables and the points: olmc_extrema_qmc's refusals
    refused(library, call(construction=2), "bad construction")
    refused(library, call(construction=-1), "bad construction")
    refused(library, call(steps=1025), "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates")
    refused(library, call(sv=False), "null pointer")
    refused(library, call(shift=False), "null pointer")
    refused(library, call(bits=32), "only 30-bit Sobol tables (SciPy's default) are supported")
    refused(library, call(steps=0), "dims must be in [1, 21201]")
    refused(library, call(steps=21202, construction=0), "dims must be in [1, 21201]")
    refused(library, call(n=0), "n_paths must be >= 1")
    refused(library, call(n=(1 << 30) + 1, steps=1), "at most 2**30 Sobol points")
    if entry != "olvq_paths":
        refused(library, call(offset=-1), "path_offset must be >= 0")
        refused(library, call(offset=1 << 30, n=1), "at most 2**30 Sobol points")
    if entry == "olvq_surface_prices":
        refused(library, call(k=0), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        refused(library, call(k=17), "the number of cells must be in [1, OLMC_MAX_BATCH]")
        sts = (_hip.Stats * 2)()
        tables = (C.c_uint32 * 64)()
        strikes, steps = (C.c_double * 2)(100.0, 100.0), (C.c_int32 * 2)(1, 5)
        refused(library, library.olvq_surface_prices(100.0, 1.0, 0.05, 0.0, 1, C.byref(good), strikes, steps, 2, 1, 0, 100, 4, tables, tables, 30, 0,
                                                             sts), "a cell's step must be in [1, n_steps]")
    if entry == "olvq_paths":
        refused(library, call(n=1 << 30, steps=8), "path matrix would exceed 64 GB")
    # two faults at once: the table, the payoff, the Sobol call (construction, bridge cap, tables, bits, points), the cells, the matrix
    one_node, keep_one = surface(n_x=1)
    refused(library, call(s=C.byref(one_node), construction=2), "n_x must be in [2, 256]")
    refused(library, call(construction=2, bits=32), "bad construction")
    refused(library, call(bits=32, n=0), "only 30-bit Sobol tables (SciPy's default) are supported")
    if entry == "olvq_price":
        refused(library, call(payoff=9, construction=2), "bad payoff")
        refused(library, call(s=C.byref(one_node), payoff=9), "n_x must be in [2, 256]")
    if entry == "olvq_surface_prices":
        refused(library, call(bits=32, k=17), "only 30-bit Sobol tables (SciPy's default) are supported")
        refused(library, call(construction=2, k=0), "bad construction")
    if entry == "olvq_paths":
        refused(library, call(construction=2, n=1 << 30, steps=8), "bad construction")
        refused(library, call(bits=32, n=1 << 30, steps=8), "only 30-bit Sobol tables (SciPy's default) are supported")
    assert keep_one is not None
    assert keep is not None and keep_bad is not None


# ------------------------------------------------------------------------------------------------------------ Python ----
def test_python_surface_of_the_qmc_model():
    assert ol.DupireLocalVolQMC is ol.local_vol.DupireLocalVolQMC and "DupireLocalVolQMC" in ol.__all__ and issubclass(ol.DupireLocalVolQMC, ol.DupireLocalVol)
    sig = inspect.signature(ol.DupireLocalVolQMC.__init__)
    assert list(sig.parameters)[1:] == ["r", "q", "n_paths", "n_steps", "seed", "path_construction"]
    assert sig.parameters["n_paths"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["n_paths"].default == 1 << 14
    assert sig.parameters["path_construction"].default == "bridge"
    for name in ("price", "price_monte_carlo", "price_asian", "price_barrier", "price_lookback", "price_surface", "simulate_paths", "local_vol_table"):
        assert inspect.signature(getattr(ol.DupireLocalVolQMC, name)) == inspect.signature(getattr(ol.DupireLocalVol, name)), name
    assert list(inspect.signature(ol.DupireLocalVol.qmc).parameters) == ["self", "path_construction"]

    strikes, expiries, iv = ol.create_sample_iv_surface()
    base = ol.DupireLocalVol(r=0.03, q=0.01, n_paths=777, n_steps=21, seed=5)
    calibrated = base.calibrate(strikes, expiries, iv, 100.0)
    for construction in ("bridge", "sequential"):
        view = base.qmc(construction)
        assert type(view) is ol.DupireLocalVolQMC and view.path_construction == construction
        assert view._calibrated is calibrated and view._spline is base._spline
        assert (view.r, view.q, view.n_paths, view.n_steps, view.seed) == (0.03, 0.01, 777, 21, 5)
        assert np.array_equal(view.local_vol_table(100.0, 1.0)[0], base.local_vol_table(100.0, 1.0)[0])
    assert base.qmc().path_construction == "bridge"

    with pytest.raises(ValueError, match="path_construction"):
        ol.DupireLocalVolQMC(path_construction="diagonal")
    with pytest.raises(ValueError, match="path_construction"):
        base.qmc("diagonal")
    # raised by exotic._qmc_tables before the device is touched
    with pytest.raises(ValueError, match="at most 1024 steps"):
        base.qmc().price_monte_carlo(100, 100, 1.0, 0.05, n_steps=1025)
    with pytest.raises(ValueError, match="at most 1024 steps"):
        base.qmc().simulate_paths(100, 1.0, 0.05, n_paths=10, n_steps=1025)
    with pytest.raises(ValueError, match="at most 21201 steps"):
        base.qmc("sequential").price_asian(100, 100, 1.0, 0.05, n_steps=21202)
    with pytest.raises(ValueError, match="at most 21201 steps"):
        base.qmc("sequential").price_surface(100, [100.0], [1.0], 0.05, n_steps=21202)
    with pytest.raises(ValueError, match="2\\*\\*30"):
        base.qmc().price_lookback(100, 100, 1.0, 0.05, n_paths=(1 << 30) + 1, n_steps=4)
    with pytest.raises(ValueError):
        base.qmc().price_barrier(100, 100, 1.0, 0.05, 0.0)
    with pytest.raises(ValueError):
        base.qmc().price_monte_carlo(100, 100, 1.0, 0.05, n_paths=0)


# ------------------------------------------------------------------------------------------------------------ oracle ----
@pytest.mark.parametrize("n", (1, 2, 13, 64, 65))
def test_oracle_composition_on_a_flat_table_is_the_gbm_reference(n):
    z = g.normals(257, n)
    S, T, r, q, sigma = 100.0, 0.75, 0.05, 0.01, 0.25              # 0.25 is exact in fp32
    flat = lvo.Table(np.full((3, 7), sigma), -0.3, 0.2, 0.5)
    for bridge in (False, True):
        got = lvo.paths(g.increments(z, bridge), flat, S, T, r, q)
        want = sr.gbm_prices(z, bridge, S, T, r, sigma, q)
        assert got.shape == want.shape == (257, n + 1)
        assert np.max(np.abs(got - want) / want) <= 1e-12, (n, bridge)
    assert np.array_equal(g.increments(-z, True), -g.increments(z, True))          # the mirror leg's increments are the negated ones, bit for bit


def test_cases_cover_every_size_once_per_table_and_once_per_point_count():
    assert len(g.CASES) == len(set(g.CASES)) == 4 * 8
    for n in g.STEPS + (g.SEQUENTIAL_ONLY_STEPS,):
        mine = [c for c in g.CASES if c[2] == n]
        assert sorted(c[0] for c in mine) == sorted(g.TABLES) and sorted(c[1] for c in mine) == sorted(g.POINTS)
    assert g.constructions(1024) == (False, True) and g.constructions(1025) == (False,)


@pytest.mark.parametrize("name", g.NAMES)
def test_no_path_of_the_gpu_cases_comes_near_a_barrier_level(name):
    """What tests/test_gpu_local_vol_qmc.py's payoff ties rest on: barrier payoffs are discontinuous at the level, so a path within
    rounding of one could tie differently on the device.  None is: the GPU test excludes nothing."""
    table = g.TABLES[name]
    shapes = [(N, n) for _name, N, n in g.CASES if _name == name] + ([(N, 64) for N in g.POINTS] if name in ("33x128", "2x7-narrow") else [])
    for N, n in shapes:
        for bridge in g.constructions(n):
            plain, mirror = g.oracle(name, N, n, bridge)
            both = np.concatenate([plain, mirror])
            for level in (g.UP, g.DOWN):
                assert np.min(np.abs(np.log(both / level))) > 1e-9, (name, N, n, bridge, level)
            if name == "2x7-narrow" and N >= 65:
                x = np.log(plain / g.S)
                assert np.mean((x > table.x_hi).any(axis=1)) >= 0.01 and np.mean((x < table.x_lo).any(axis=1)) >= 0.01, (N, n, bridge)


def test_black_scholes_gap_of_the_flat_case_is_below_a_thousandth():
    for is_call in (True, False):
        assert g.black_scholes_gap_of_the_oracle(is_call) <= 1e-3


# ----------------------------------------------------------------------------------------------------------- scatter ----
def test_sobol_points_shrink_the_scatter_of_smooth_payoffs():
    table = g.TABLES["33x128"]
    N, n = 1 << 12, 64
    price = lambda dw, code: float(np.exp(-g.R * g.T) * np.mean(lvo.payoff(lvo.paths(dw, table, g.S, g.T, g.R, g.Q), code, True, g.K)))
    runs = {"pseudo": [], "sequential": [], "bridge": []}
    for s in range(16):
        z = g.normals(N, n, seed=s)
        runs["pseudo"].append([price(np.random.default_rng(1000 + s).standard_normal((N, n)), code) for code in (6, 8)])
        runs["sequential"].append([price(z, code) for code in (6, 8)])
        runs["bridge"].append([price(g.increments(z, True), code) for code in (6, 8)])
    std = {k: np.std(np.array(v), axis=0, ddof=1) for k, v in runs.items()}
    for j, code in enumerate((6, 8)):
        bridge, sequential = std["pseudo"][j] / std["bridge"][j], std["pseudo"][j] / std["sequential"][j]
        print(f"SCATTER code {code}: pseudo / bridge {bridge:.1f}, pseudo / sequential {sequential:.1f}")
        assert bridge >= 10.0 and sequential >= 3.0, (code, bridge, sequential)
