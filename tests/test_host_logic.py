"""Host-side mirror of the reference API (no GPU needed): constructor contract,
expired-option early-out, the generic FD Greeks driver, adapters, Black-Scholes,
and the rule that the product never reaches into oracle/."""
import os
import re

import pytest

import optionslab_amd as ol
from optionslab_amd.greeks import fd_steps
from oracle import numpy_reference as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_contract():          # reference tests/test_monte_carlo.py:95-112
    p = ol.MonteCarloPricer(num_simulations=5000, num_steps=100, seed=123)
    assert (p.num_simulations, p.num_steps, p.seed) == (5000, 100, 123)
    assert p.method == ol.MCMethod.NUMPY
    for bad in (0, -100):
        with pytest.raises(ValueError):
            ol.MonteCarloPricer(num_simulations=bad)
    q = ol.MonteCarloPricer()
    assert (q.num_simulations, q.num_steps) == (100000, 1) and 0 <= q.seed < 2**31
    with pytest.raises(AttributeError):   # __slots__, monte_carlo.py:54
        p.extra = 1


def test_n_gpus_is_additive_and_keyword_only():
    """The multi-GPU switch of the pricer: keyword only, default 1, validated; the reference's positional contract
    (num_simulations, num_steps, seed, method) is untouched."""
    p = ol.MonteCarloPricer(5000, 100, 123, ol.MCMethod.NUMPY)
    assert p.n_gpus == 1
    assert ol.MonteCarloPricer(5000, 100, 123, n_gpus=8).n_gpus == 8
    with pytest.raises(TypeError):
        ol.MonteCarloPricer(5000, 100, 123, ol.MCMethod.NUMPY, 8)          # not a fifth positional argument
    with pytest.raises(ValueError):
        ol.MonteCarloPricer(5000, n_gpus=0)
    assert ol.MonteCarloPricer(5000, 16, 1, ol.MCMethod.QMC, n_gpus=2).n_gpus == 2       # round 5: the Sobol price shards its points too
    assert ol.MonteCarloPricer(1000, 10, 1, n_gpus=4).price(120, 100, 0.0, 0.05, 0.2, "call") == 20     # T <= 0: no device, whatever n_gpus


def test_method_enum_keeps_reference_members():
    assert {m.value for m in ol.MCMethod} >= {"numpy", "numba", "qmc", "fast"}
    assert ol.MCMethod("hip") is ol.MCMethod.HIP
    assert ol.NUMBA_AVAILABLE is False


def test_expired_option_returns_intrinsic_without_simulating(golden):
    p = ol.MonteCarloPricer(1000, 10, 1)
    for e in golden["expired"]:
        S, K, T, r, v, typ = e["args"]
        res = p.price(S, K, T, r, v, typ, return_error=True)
        assert isinstance(res, ol.MCResult)
        assert (res.price, res.std_error, res.n_paths) == (e["price"], 0.0, 0)
        assert p.price(S, K, T, r, v, typ) == e["plain"]


def test_mcresult_defaults():
    r = ol.MCResult(1.5)
    assert (r.price, r.std_error, r.n_paths) == (1.5, 0.0, 0)


def test_black_scholes_matches_reference(golden):
    for row in golden["black_scholes"]:
        S, K, T, r, v, q = row["args"]
        assert ol.black_scholes(S, K, T, r, v, "call", q) == pytest.approx(row["call"], rel=1e-13, abs=1e-13)
        assert ol.black_scholes(S, K, T, r, v, "put", q) == pytest.approx(row["put"], rel=1e-13, abs=1e-13)
    with pytest.raises(ValueError):
        ol.black_scholes(100, -1, 1, 0.05, 0.2)
    with pytest.raises(ValueError):
        ol.black_scholes(100, 100, 1, 0.05, 0.2, "strangle")


class AnalyticPricer:
    """PricerProtocol-conforming stand-in: counts calls, prices with BSM."""

    def __init__(self):
        self.calls = []

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kw):
        self.calls.append((S, K, T, r, sigma, q))
        return float(orc.bs_price(S, K, T, r, sigma, option_type, q))


@pytest.mark.parametrize("second,n_calls", [(False, 8), (True, 14)])
def test_generic_fd_driver_equals_reference_driver(second, n_calls):
    pr = AnalyticPricer()
    assert isinstance(pr, ol.PricerProtocol)
    g = ol.compute_greeks_unified(pr, 100.0, 100.0, 1.0, 0.05, 0.2, "call", 0.0, include_second_order=second)
    want = orc.fd_greeks(AnalyticPricer().price, 100.0, 100.0, 1.0, 0.05, 0.2, "call", 0.0, include_second_order=second)
    assert list(g.keys()) == list(want.keys())
    assert all(g[k] == want[k] for k in g)                      # same bumps, same arithmetic order
    assert len(pr.calls) == n_calls == len(set(pr.calls))       # memo: every tuple priced once
    exact = orc.bs_greeks(100.0, 100.0, 1.0, 0.05, 0.2, "call")
    assert g["delta"] == pytest.approx(exact["delta"], abs=1e-4)
    assert g["vega"] == pytest.approx(exact["vega"], rel=1e-3)
    assert g["rho"] == pytest.approx(exact["rho"], rel=1e-4)


def test_fd_driver_short_dated_branch_and_bump_sizes():
    assert fd_steps(100.0) == (1.0, 0.01, 1e-4, 1 / 365.0)
    assert fd_steps(0.001)[0] == 1e-4
    pr = AnalyticPricer()
    g = ol.compute_greeks_unified(pr, 100.0, 100.0, 0.002, 0.05, 0.2, "call")
    want = orc.fd_greeks(AnalyticPricer().price, 100.0, 100.0, 0.002, 0.05, 0.2, "call")
    assert g["theta"] == want["theta"] == -g["price"] / 0.002 and g["charm"] == 0.0
    assert len(pr.calls) == 11


def test_fd_driver_wraps_errors_in_greeks_error():
    class Broken:
        def price(self, *a, **k):
            raise RuntimeError("boom")

    with pytest.raises(ol.GreeksError) as e:
        ol.compute_greeks_unified(Broken(), 100, 100, 1.0, 0.05, 0.2)
    assert "boom" in str(e.value) and isinstance(e.value.__cause__, RuntimeError)
    with pytest.raises(ol.GreeksError):   # fused form needs the device pricer
        ol.compute_greeks_unified(AnalyticPricer(), 100, 100, 1.0, 0.05, 0.2, fused=True)


def test_exotic_adapter_reparameterises_and_forwards_kwargs():
    class Probe:
        S = K = T = r = sigma = q = None

        def price(self, n_paths, n_steps, **kw):
            self.seen = (n_paths, n_steps, kw)
            return self.S - self.K

    ad = ol.ExoticAdapter(Probe(), n_paths=123, n_steps=7, avg_type="geometric")
    assert ad.price(110.0, 100.0, 0.5, 0.01, 0.3, "put", 0.02) == 10.0
    assert ad.exotic.seen == (123, 7, {"avg_type": "geometric", "option_type": "put"})
    assert (ad.exotic.T, ad.exotic.r, ad.exotic.sigma, ad.exotic.q) == (0.5, 0.01, 0.3, 0.02)


def test_asian_closed_form_matches_reference(golden):
    for c in golden["asian"]:
        S, K, T, r, v, q = c["params"]
        got = ol.AsianOption(S, K, T, r, v, q).price_geometric_closed_form(c["option_type"])
        assert got == pytest.approx(c["geometric_closed_form"], rel=1e-13)


def test_exception_hierarchy():
    assert issubclass(ol.AccelerationError, ol.MonteCarloError)
    assert issubclass(ol.InputValidationError, ol.MonteCarloError)
    e = ol.AccelerationError("x", backend="hip")
    assert e.backend == "hip" and "backend: hip" in str(e)
    assert "after 5 iterations" in str(ol.ConvergenceError("y", iterations=5))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "optionslab_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
                assert "numpy_reference" not in text and "philox_oracle" not in text and "oracle/" not in text, f


def test_importing_the_package_loads_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys, optionslab_amd, optionslab_amd._hip as h; "
            "assert 'torch' not in sys.modules; assert h._lib is None; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.stdout.strip() == "ok", out.stderr


def test_compat_install_makes_reference_import_paths_resolve_here():
    import importlib
    import sys

    from optionslab_amd import compat

    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    try:
        compat.install()
        compat.install()                                      # idempotent
        mc = importlib.import_module("src.pricing_models.monte_carlo")
        from src.greeks.unified_greeks import compute_greeks_unified          # noqa: F401  (the reference's import lines)
        from src.pricing_models.black_scholes import black_scholes
        from src.pricing_models.monte_carlo import NUMBA_AVAILABLE, MCMethod, MonteCarloPricer
        from src.pricing_models.monte_carlo_unified import InputValidationError as UniErr
        from src.pricing_models.monte_carlo_unified import MonteCarloPricerUni
        from src.simulation import simulate_gbm_numpy
        # package-level re-exports of the reference's __init__ files (src/pricing_models/__init__.py:23-66, src/greeks/__init__.py:11-23)
        from src.greeks import HestonAdapter, JumpDiffusionAdapter, greeks_heston
        from src.greeks import compute_greeks_unified as cgu
        from src.pricing_models import AsianOption, HestonPricer, KouJumpDiffusion
        from src.pricing_models import MonteCarloPricer as PackageLevelPricer
        from src.pricing_models import GPU_AVAILABLE, black_scholes as page_bs          # streamlit_app/pages/1_MonteCarlo_Basic.py:51-57
        from src.simulation.gbm_numpy import simulate_gbm_paths
        assert GPU_AVAILABLE is True and page_bs is black_scholes
        from src.simulation.gbm_qmc import simulate_gbm_qmc_antithetic
        assert PackageLevelPricer is ol.MonteCarloPricer and cgu is compute_greeks_unified and AsianOption is ol.AsianOption
        assert HestonPricer is ol.HestonPricer and KouJumpDiffusion is ol.KouJumpDiffusion and HestonAdapter is ol.HestonAdapter
        assert JumpDiffusionAdapter is ol.JumpDiffusionAdapter and greeks_heston is ol.greeks_heston
        assert simulate_gbm_paths is ol.simulate_gbm_paths_hip and simulate_gbm_qmc_antithetic is ol.simulate_gbm_qmc_antithetic_hip
        assert MonteCarloPricer is ol.MonteCarloPricer and MCMethod is ol.MCMethod and NUMBA_AVAILABLE is False
        assert mc.MonteCarloPricer(num_simulations=10, num_steps=5, seed=1).price(120, 100, 0.0, 0.05, 0.2, "call") == 20
        assert black_scholes(100, 100, 1.0, 0.05, 0.2) == ol.black_scholes(100, 100, 1.0, 0.05, 0.2)
        assert simulate_gbm_numpy is ol.simulate_gbm_hip
        with pytest.raises(UniErr):
            MonteCarloPricerUni(num_simulations=0)
    finally:
        compat.uninstall()
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert "src.pricing_models.monte_carlo" not in sys.modules or not getattr(sys.modules["src.pricing_models.monte_carlo"], "__optionslab_amd__", False)


# ---- MCMethod.QMC leans on SciPy privates (Sobol._sv / ._shift): the guard around them ----
def test_sobol_tables_reproduce_scipys_own_points():
    import numpy as np
    from scipy.stats.qmc import Sobol
    from optionslab_amd import monte_carlo as mc

    mc._sobol_cache.clear()
    sv, shift = mc.sobol_tables(16, 42)                      # passes the behavioural self-check on construction
    assert sv.shape == (16, 30) and shift.shape == (16,) and sv.dtype == np.uint32
    pts = Sobol(d=16, scramble=True, seed=42).random(64)     # gbm_qmc.py:32-33
    assert np.array_equal(mc.expand_sobol_points(sv, shift, 0, 64), pts)
    assert np.array_equal(mc.expand_sobol_points(sv, shift, 37, 5), pts[37:42])
    import scipy
    assert mc.SOBOL_VALIDATED_SCIPY.count(".") == 2
    if scipy.__version__ != mc.SOBOL_VALIDATED_SCIPY:        # another SciPy is fine exactly as long as the check above held
        assert np.array_equal(mc.expand_sobol_points(sv, shift, 0, 8), pts[:8])


@pytest.mark.parametrize("privates", ["absent", "reordered_columns"])
def test_sobol_tables_are_derived_from_public_behaviour_when_the_privates_fail(monkeypatch, privates):
    """A SciPy that drops or re-lays-out `_sv` / `_shift` but keeps the public engine (.random, .fast_forward, 30 bits) does not
    switch MCMethod.QMC off: consecutive points of the Gray-code sequence differ by one column of the direction matrix, so the
    tables are read off the engine's own points -- and are the very tables the privates hold, column by column, for every column
    the asked number of points can select (the rest stay zero)."""
    import numpy as np
    from scipy.stats import qmc
    from optionslab_amd import monte_carlo as mc

    real = qmc.Sobol

    class PublicOnly:
        bits = 30

        def __init__(self, d, scramble=True, seed=None):
            self._eng = real(d=d, scramble=scramble, seed=seed)
            if privates == "reordered_columns":
                self._sv, self._shift = np.array(self._eng._sv)[:, ::-1], np.array(self._eng._shift)

        def random(self, n):
            return self._eng.random(n)

        def fast_forward(self, n):
            self._eng.fast_forward(n)
            return self

    monkeypatch.setattr(qmc, "Sobol", PublicOnly)
    mc._sobol_cache.clear()
    sv, shift = mc.sobol_tables(12, 5, n_points=3000)            # 12 columns can be selected by point indices below 4096
    truth = real(d=12, scramble=True, seed=5)
    assert np.array_equal(shift, np.asarray(truth._shift, dtype=np.uint32))
    assert np.array_equal(sv[:, :12], np.asarray(truth._sv, dtype=np.uint32)[:, :12]) and not sv[:, 12:].any()
    pts = truth.random(3000)
    assert np.array_equal(mc.expand_sobol_points(sv, shift, 2990, 10), pts[2990:])
    # asking for more points later derives more columns (and replaces the cached, shorter tables)
    sv2, _ = mc.sobol_tables(12, 5, n_points=1 << 15)
    assert np.array_equal(sv2[:, :15], np.asarray(truth._sv, dtype=np.uint32)[:, :15]) and not sv2[:, 15:].any()
    assert mc.sobol_tables(12, 5, n_points=100)[0] is sv2        # fewer points: the cached tables serve
    # the tables know how many columns they hold: a point range that reaches beyond them is refused before any launch,
    # instead of silently repeating points (the zero columns select nothing)
    assert sv.valid_bits == 12 and sv2.valid_bits == 15
    from optionslab_amd import _hip
    with pytest.raises(ValueError, match="beyond the 2\\*\\*12 points"):
        _hip.european_qmc(100.0, 100.0, 1.0, 0.05, 0.2, 0.0, True, 4000, sv, shift, point_offset=200)
    with pytest.raises(ValueError, match="beyond the 2\\*\\*15 points"):
        _hip.european_qmc_greeks_fd(100.0, 100.0, 1.0, 0.05, 0.2, 0.0, True, (1 << 15) + 1, sv2, shift, True)
    monkeypatch.setattr(qmc, "Sobol", real)
    mc._sobol_cache.clear()
    full = mc.sobol_tables(12, 5)[0]
    assert np.array_equal(full, np.asarray(truth._sv, dtype=np.uint32)) and full.valid_bits == 30       # the private tables, all 30 columns


@pytest.mark.parametrize("breakage", ["no_tables", "wrong_bits", "reordered_columns", "wrong_shape"])
def test_sobol_guard_refuses_an_engine_whose_private_tables_changed(monkeypatch, breakage):
    """A SciPy bump that removes or re-lays-out the private tables AND offers no .fast_forward() to derive them from (or is not the
    30-bit engine) must disable QMC loudly (AccelerationError), never price on other points: the guard checks behaviour, not just
    attribute names."""
    import numpy as np
    from scipy.stats import qmc
    from optionslab_amd import monte_carlo as mc

    real = qmc.Sobol

    class Stub:
        def __init__(self, d, scramble=True, seed=None):
            self._eng = real(d=d, scramble=scramble, seed=seed)
            self.bits = 30 if breakage != "wrong_bits" else 64
            if breakage != "no_tables":
                sv = np.array(self._eng._sv)
                if breakage == "reordered_columns":
                    sv = sv[:, ::-1]                         # same name, same shape, different meaning
                if breakage == "wrong_shape":
                    sv = sv[:, :20]
                self._sv, self._shift = sv, np.array(self._eng._shift)

        def random(self, n):
            return self._eng.random(n)

    monkeypatch.setattr(qmc, "Sobol", Stub)
    mc._sobol_cache.clear()
    with pytest.raises(ol.AccelerationError) as e:
        mc.sobol_tables(12, 5)
    assert e.value.backend == "hip" and mc.SOBOL_VALIDATED_SCIPY in str(e.value)
    assert not mc._sobol_cache                               # nothing bad was cached
    monkeypatch.setattr(qmc, "Sobol", real)
    assert mc.sobol_tables(12, 5)[0].shape == (12, 30)       # and the real engine still works afterwards


# ---- layout of a contract set for the fused kernels (host arithmetic of libolmc, no device) ---------------------------------------
def _layout_invariants(opts, n_steps):
    import math
    from optionslab_amd import _hip
    nsets, pos, mask, cont, scale = _hip.contract_layout(opts, n_steps)
    k, H = len(opts), (8 if len(opts) <= 8 else 16) // 2
    assert nsets == 2 * H and sorted(pos) == sorted(set(pos)) and all(0 <= p < nsets for p in pos)          # distinct slots
    assert mask & 1, "slot 0 is always a base"
    slot_of = {p: i for i, p in enumerate(pos)}

    def consts(o):
        S, K, T, r, v, q, _c = o
        dt = T / n_steps
        return math.log(S) + (r - q - 0.5 * v * v) * dt * n_steps, v * math.sqrt(dt)

    # the second half starts with a base, or continues slot 0's group -- and then no other base sits between slot 0 and the middle
    if cont:
        assert not (mask >> H) & 1 and not any((mask >> s) & 1 for s in range(1, H))
    else:
        assert (mask >> H) & 1
    for half in (range(0, H), range(H, nsets)):
        base = 0 if (cont and half[0] == H) else None
        for s in half:
            if (mask >> s) & 1:
                base = s
                assert scale[s] == 1.0
            elif s in slot_of:                      # a real (not padding) contract that takes scale * S_T(base)
                assert base is not None and base in slot_of or base == 0
                a, vol = consts(opts[slot_of[s]])
                a_b, vol_b = consts(opts[slot_of[base]])
                assert vol == vol_b, "a scaled contract shares its base's vol bit for bit"
                assert scale[s] == pytest.approx(math.exp(a - a_b), rel=1e-15)
    # contracts with one vol sit in consecutive slots (a group), up to the forced split at the middle
    groups = {}
    for i, o in enumerate(opts):
        groups.setdefault(consts(o)[1], []).append(pos[i])
    for slots in groups.values():
        assert sorted(slots) == list(range(min(slots), min(slots) + len(slots)))
    return nsets, pos, mask, cont


def test_contract_set_layout_of_the_greeks_sets_and_of_random_sets():
    """group_contracts (olmc.hip): what the fused kernels' two-stream walk relies on.  First-order Greeks: {mid, S+, S-, r+, r-} is
    slot 0's group and straddles the middle of the 8-slot set -> the second stream continues it (no base of its own there); second
    order: 14 contracts, 4 groups, slot 8 is a natural base."""
    S, K, T, r, v, q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0
    h_S, h_v, h_r, h_T = 1.0, 0.01, 1e-4, 1 / 365.0
    first = [(S, K, T, r, v, q, True), (S + h_S, K, T, r, v, q, True), (S - h_S, K, T, r, v, q, True), (S, K, T, r, v + h_v, q, True),
             (S, K, T, r, v - h_v, q, True), (S, K, T - h_T, r, v, q, True), (S, K, T, r + h_r, v, q, True), (S, K, T, r - h_r, v, q, True)]
    nsets, pos, mask, cont = _layout_invariants(first, 252)
    assert nsets == 8 and cont and pos[:3] == [0, 1, 2] and sorted(pos[i] for i in (0, 1, 2, 6, 7)) == [0, 1, 2, 3, 4]
    assert bin(mask).count("1") == 4                                              # mid, sigma+, sigma-, T-: four pairs of exponentials
    second = first + [(S + h_S, K, T, r, v + h_v, q, True), (S + h_S, K, T, r, v - h_v, q, True), (S - h_S, K, T, r, v + h_v, q, True),
                      (S - h_S, K, T, r, v - h_v, q, True), (S + h_S, K, T - h_T, r, v, q, True), (S - h_S, K, T - h_T, r, v, q, True)]
    nsets, pos, mask, cont = _layout_invariants(second, 252)
    assert nsets == 16 and not cont and bin(mask & ((1 << 14) - 1)).count("1") == 4
    import numpy as np
    rng = np.random.default_rng(5)
    for _ in range(300):
        k = int(rng.integers(2, 17))
        vols = [0.1 + 0.05 * g for g in range(int(rng.integers(1, 7)))]
        opts = [(100.0 + float(rng.normal(0, 3)), float(rng.uniform(80, 120)), 1.0, 0.05 + float(rng.normal(0, 0.01)), vols[int(rng.integers(0, len(vols)))], 0.0,
                 bool(rng.integers(0, 2))) for _ in range(k)]
        _layout_invariants(opts, int(rng.integers(1, 300)))


def test_reference_barrier_level_reproduces_the_reference_t0_decision():
    """BarrierOption passes the C ABI a level whose log-space t = 0 decision (0 against ln(level/S): a level at the spot is crossed)
    is the reference's on its column 0, np.exp(np.log(S)); the level stays within a few ulps of the contract's."""
    import numpy as np
    from optionslab_amd.exotic import reference_barrier_level

    spots = [100.0, 80.0, 95.0, 110.0, 120.0, 3.0, 50.0] + list(np.random.default_rng(5).uniform(1.0, 500.0, 300))
    moved = 0
    for S in spots:
        s0 = np.exp(np.full(3, np.log(S)))[0]
        for B in (S, np.nextafter(S, 0.0), np.nextafter(S, np.inf), 0.9 * S, 1.1 * S):
            for kind in ("up-and-out", "up-and-in", "down-and-out", "down-and-in"):
                up = kind.startswith("up")
                level = reference_barrier_level(S, B, kind)
                assert ((level / S <= 1.0) if up else (level / S >= 1.0)) == ((s0 >= B) if up else (s0 <= B)), (S, B, kind)
                assert abs(level - B) <= 8 * np.spacing(B) and (level == B or abs(B - S) <= 4 * np.spacing(S))
                moved += level != B
    assert moved > 0                                                    # 100 and 80 need a nudge (100: down; 80: up)
    assert reference_barrier_level(95.0, 95.0, "down-and-out") == 95.0
    assert reference_barrier_level(100.0, 100.0, "down-and-out") < 100.0 and reference_barrier_level(80.0, 80.0, "up-and-out") > 80.0
