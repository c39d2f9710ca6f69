"""Heston's quadratic-exponential scheme without a GPU: the NumPy restatement's defining properties (tests/heston_qe_reference.py is what
tests/test_gpu_heston_qe.py ties the device to) and the host logic of the `scheme` keyword.

1. Moment matching: mean and variance of v' equal m and s^2 in both branches, to 1e-6 relative, by quadrature over the draw.
2. v' >= 0, and v' = 0 exactly where U_v <= p.
3. sigma_v -> 1e-6 reproduces Black-Scholes paths to 1e-5.
4. Host logic: the refusals before the device, scheme="euler" on today's bindings, scheme="qe" on the new ones, the one-cell routing.
5. The C ABI: declared, bound, exported, and its refusals before any device work.
"""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
from scipy.special import ndtr

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd import heston as hes
from tests import heston_qe_reference as qe
from tests.abi_support import library, no_library, refused, sobol as _sobol
from tests.gpu_support import heston_pricer as pricer

S, R, Q, T = 100.0, 0.05, 0.0, 1.0
QE_NAMES = ("olmc_heston_qe_surface", "olmc_heston_qe_qmc_surface", "olmc_heston_qe_paths", "olmc_heston_qe_qmc_paths")


# ---------------------------------------------------------------------------------------------------- 1. the moments ----
@pytest.mark.parametrize("n", (4, 16))
@pytest.mark.parametrize("name", sorted(qe.MODELS))
def test_the_next_variance_has_the_exact_conditional_mean_and_variance(name, n):
    """The defining property of QE.  Quadrature over the draw the branch reads, through next_variance itself:
    quadratic -- Gauss-Hermite nodes z (64 nodes, weight exp(-z^2 / 2): exact for the quartic (b + z)^4), fed as z_v with u_v = Phi(z);
    exponential -- v' = 0 on U <= p, and on U > p the substitution U = 1 - (1 - p) exp(-x) turns E[v'^k] into (1 - p) times a
    Gauss-Laguerre sum (8 nodes, the largest 22.9: exact for x and x^2), fed as u_v."""
    model = qe.MODELS[name]
    theta = model[1]
    c = qe.constants(model, R, Q, T, n)
    z, wz = np.polynomial.hermite_e.hermegauss(64)
    wz = wz / math.sqrt(2.0 * math.pi)
    x, wx = np.polynomial.laguerre.laggauss(8)
    branches = set()
    for v in (0.0, theta / 10, theta, 5 * theta):
        m, s2, psi = (float(a) for a in qe.moments(v, c))
        if psi <= qe.PSI_C:
            vn, quadratic = qe.next_variance(np.full_like(z, v), ndtr(z), z, c)
            assert quadratic.all()
            mean, second = float(np.sum(wz * vn)), float(np.sum(wz * vn * vn))
        else:
            p = float(qe.exponential_p(v, c))
            u = 1.0 - (1.0 - p) * np.exp(-x)
            vn, quadratic = qe.next_variance(np.full_like(u, v), u, np.zeros_like(u), c)
            assert not quadratic.any() and np.all(u > p)
            mean, second = (1.0 - p) * float(np.sum(wx * vn)), (1.0 - p) * float(np.sum(wx * vn * vn))
        branches.add(psi <= qe.PSI_C)
        print(name, n, v, "psi", psi, "mean", mean, m, "variance", second - mean * mean, s2)
        assert mean == pytest.approx(m, rel=1e-6)
        assert second - mean * mean == pytest.approx(s2, rel=1e-6)
    assert branches == ({True} if name == "usual" else {True, False})


def test_at_zero_variance_psi_is_sigma_squared_over_two_kappa_theta():
    for model in qe.MODELS.values():
        kappa, theta, sigma_v = model[:3]
        m, s2, psi = qe.moments(0.0, qe.constants(model, R, Q, T, 16))
        assert float(m) > 0.0 and float(s2) > 0.0
        assert float(psi) == pytest.approx(sigma_v**2 / (2 * kappa * theta), rel=1e-12)


# ------------------------------------------------------------------------------------- 2. non-negative, zero below p ----
def test_the_next_variance_is_never_negative_and_zero_exactly_below_p():
    rng = np.random.default_rng(11)
    for model in qe.MODELS.values():
        c = qe.constants(model, R, Q, T, 16)
        v = np.concatenate([np.zeros(1000), rng.gamma(0.5, 2 * model[1], 99_000)])
        u = (rng.integers(0, 1 << 32, v.size, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0**-32
        z = rng.standard_normal(v.size)
        for leg_u, leg_z in ((u, z), (1.0 - u, -z)):
            vn, quadratic = qe.next_variance(v, leg_u, leg_z, c)
            assert np.all(vn >= 0.0) and np.all(np.isfinite(vn))
            p = qe.exponential_p(v, c)
            exponential = ~quadratic
            assert np.array_equal(vn[exponential] == 0.0, leg_u[exponential] <= p[exponential])
            if exponential.any():
                assert np.any(vn[exponential] == 0.0) and np.any(vn[exponential] > 0.0)
                assert np.all(p[exponential] > 0.2 - 1e-12)                         # psi > 1.5


# --------------------------------------------------------------------------------------- 3. the Black-Scholes limit ----
def test_a_vanishing_vol_of_vol_reproduces_black_scholes_paths():
    """theta = v0 and sigma_v = 1e-6: the variance stays at v0 and ln S follows a Brownian motion of volatility sqrt(v0) driven by
    rho Z_v + sqrt(1 - rho^2) Z_s.  The variance's noise is an exact Ornstein-Uhlenbeck step, so the Brownian increment the spot sees
    through K1, K2 is sqrt(dt) Z_v (1 + O((kappa dt)^2)): kappa dt = 1/160 keeps that factor's effect on a path (about 4e-5 of a
    log-return of a few tenths) below the 1e-5 asked of the limit; the terms of order sigma_v are near 1e-7."""
    rng = np.random.default_rng(5)
    N, n, rho, sigma2 = 2000, 16, -0.7, 0.09
    model = (0.1, sigma2, 1e-6, rho, sigma2)
    u, z_s = rng.random((N, n)), rng.standard_normal((N, n))
    z_v = rng.standard_normal((N, n))
    for mirror in (False, True):
        spot, var, quadratic, _psi = qe.paths(S, model, R, 0.01, T, n, u, z_v, z_s, mirror)
        sign = -1.0 if mirror else 1.0
        w = np.cumsum(sign * (rho * z_v + math.sqrt(1 - rho * rho) * z_s), axis=1)
        dt = T / n
        t = dt * np.arange(1, n + 1)
        want = S * np.exp((R - 0.01 - 0.5 * sigma2) * t + math.sqrt(sigma2 * dt) * w)
        assert quadratic.all()
        assert float(np.max(np.abs(spot[:, 1:] / want - 1.0))) < 1e-5
        assert float(np.max(np.abs(var / sigma2 - 1.0))) < 2e-5                    # sigma_v |W_v| / sqrt(v0) at six deviations of W_v(T)
        assert np.all(spot[:, 0] == S) and np.all(var[:, 0] == sigma2)


# ------------------------------------------------------------------------------------------------- 4. the host logic ----
def test_every_entry_takes_the_keyword_and_defaults_to_euler():
    for f in (ol.HestonPricer.price_monte_carlo, ol.HestonPricer.simulate_paths, ol.HestonPricer.price_surface, hes.calibration_objective,
              hes.calibrate_heston):
        parameter = inspect.signature(f).parameters["scheme"]
        assert parameter.default == "euler" and parameter.kind is inspect.Parameter.KEYWORD_ONLY
    for f in (ol.HestonPricer.price_asian, ol.HestonPricer.price_barrier, ol.HestonPricer.price_lookback):
        assert "scheme" not in inspect.signature(f).parameters


def _market():
    return dict(spot=S, strikes=(90.0, 100.0, 110.0), maturities=(0.25, 0.5, 1.0), market_ivs=np.full((3, 3), 0.3), r=R, q=Q)


def test_the_refusals_come_before_the_device(no_library):
    p = pricer(qe.FELLER_VIOLATED)
    calls = {
        "price_monte_carlo": lambda **kw: p.price_monte_carlo(S, 100.0, T, R, Q, "call", 100, 16, 1, **kw),
        "simulate_paths": lambda **kw: p.simulate_paths(S, T, R, Q, 100, 16, 1, **kw),
        "price_surface": lambda **kw: p.price_surface(S, (100.0,), (0.5, 1.0), R, Q, "call", 100, 16, 1, **kw),
        "calibration_objective": lambda **kw: hes.calibration_objective(_market(), n_paths=128, n_steps=16, **{"method": "pseudo", **kw}),
        "calibrate_heston": lambda **kw: hes.calibrate_heston(_market(), n_paths=128, n_steps=16, **{"method": "pseudo", **kw}),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="scheme must be"):
            call(scheme="milstein")
        with pytest.raises(ValueError, match="pass path_construction='sequential'"):
            call(scheme="qe", method="qmc")                                         # the default construction is the bridge
        with pytest.raises(ValueError, match="pass path_construction='sequential'"):
            call(scheme="qe", method="qmc", path_construction="bridge")
        with pytest.raises(ValueError, match="method"):
            call(scheme="qe", method="sobol")
        with pytest.raises(ValueError, match="path_construction"):
            call(scheme="qe", method="qmc", path_construction="pca")
    with pytest.raises(ValueError, match=">= 1"):
        p.price_monte_carlo(S, 100.0, T, R, Q, "call", 0, 16, 1, scheme="qe")
    with pytest.raises(ValueError, match="0.3"):
        p.price_surface(S, (100.0,), (0.3, 1.0), R, Q, "call", 100, 16, 1, scheme="qe")
    # the calibrators accept QE on the sequential construction without touching the device
    assert callable(hes.calibration_objective(_market(), n_paths=128, n_steps=16, path_construction="sequential", scheme="qe"))


BINDINGS = ("heston", "heston_qmc", "heston_paths", "heston_qmc_paths", "heston_surface", "heston_qmc_surface", "heston_path_payoff",
            "heston_qmc_path_payoff", "heston_qe_surface", "heston_qe_qmc_surface", "heston_qe_paths", "heston_qe_qmc_paths")


@pytest.fixture
def recorded(no_library, monkeypatch):
    """Every Heston binding replaced by a recorder that answers in the binding's shape."""
    calls = []

    def recorder(name):
        def call(*args, **kw):
            calls.append((name, args, kw))
            if name.endswith("surface"):
                out = []
                for k, m in zip(args[10], args[11]):
                    st = _hip.Stats()
                    st.price, st.std_error = k + m, 0.25
                    out.append(st)
                return out
            if name.endswith("paths"):
                return np.zeros((2, 2)), np.ones((2, 2))
            st = _hip.Stats()
            st.price, st.std_error = 7.0, 0.5
            return st
        return call

    for name in BINDINGS:
        monkeypatch.setattr(_hip, name, recorder(name))
    return calls


def test_euler_calls_exactly_the_bindings_it_called_before(recorded):
    model = qe.USUAL
    p = pricer(model)
    sequential = dict(method="qmc", path_construction="sequential")
    for extra in (dict(), dict(scheme="euler")):
        recorded.clear()
        assert p.price_monte_carlo(S, 100.0, T, R, Q, "call", 1000, 16, 3, True, **extra) == 7.0
        assert p.price_monte_carlo(S, 100.0, T, R, Q, "put", 128, 16, 3, **sequential, **extra) == 7.0
        p.simulate_paths(S, T, R, Q, 1000, 16, 3, **extra)
        p.simulate_paths(S, T, R, Q, 128, 16, 3, method="qmc", **extra)
        p.price_surface(S, (90.0, 110.0), (0.5, 1.0), R, Q, "call", 1000, 16, 3, **extra)
        p.price_surface(S, (90.0, 110.0), (0.5, 1.0), R, Q, "call", 128, 16, 3, method="qmc", **extra)
        hes.calibration_objective(_market(), n_paths=128, n_steps=16, seed=3, **extra)(model)
        assert [name for name, _a, _k in recorded] == ["heston", "heston_qmc", "heston_paths", "heston_qmc_paths", "heston_surface",
                                                        "heston_qmc_surface", "heston_qmc_surface"]
        (_n, args, _k) = recorded[0]
        assert args == (S, 100.0, T, R, Q, True, *model, 1000, 16, 3, True)
        (_n, args, _k) = recorded[1]
        assert args[:11] == (S, 100.0, T, R, Q, False, *model) and args[11] == 128 and args[12].shape == (32, 30) and args[14:] == (False, False)
        (_n, args, kw) = recorded[2]
        assert args == (S, T, R, Q, *model, 1000, 16, 3) and kw == dict(path_major=True)
        (_n, args, kw) = recorded[3]
        assert args[:9] == (S, T, R, Q, *model) and args[9] == 128 and args[12] is True and kw == dict(path_major=True)
        (_n, args, _k) = recorded[4]
        assert args[:10] == (S, T, R, Q, True, *model) and args[10:] == ([90.0, 110.0, 90.0, 110.0], [8, 8, 16, 16], 1000, 16, 3, False)
        (_n, args, _k) = recorded[5]
        assert args[12] == 128 and args[15:] == (True, False)                       # the bridge, as before
        (_n, args, _k) = recorded[6]
        assert args[12] == 128 and args[13].shape == (32, 30) and args[15:] == (True, False) and len(args[10]) == 9


def test_qe_reaches_its_own_bindings_and_a_price_is_the_one_cell_surface(recorded):
    model = qe.FELLER_VIOLATED
    p = pricer(model)
    sequential = dict(method="qmc", path_construction="sequential", scheme="qe")
    # price_monte_carlo: one cell (K, n_steps) of a surface launch
    price, error = p.price_monte_carlo(S, 120.0, T, R, Q, "put", 1000, 16, 3, True, True, scheme="qe")
    (name, args, _k), = recorded
    assert name == "heston_qe_surface" and args == (S, T, R, Q, False, *model, [120.0], [16], 1000, 16, 3, True)
    assert (price, error) == (120.0 + 16, 0.25) and isinstance(price, np.float64)
    recorded.clear()
    assert p.price_monte_carlo(S, 120.0, 0.5, R, Q, "call", 128, 8, 3, **sequential) == 128.0
    (name, args, _k), = recorded
    assert name == "heston_qe_qmc_surface" and args[:12] == (S, 0.5, R, Q, True, *model, [120.0], [8])
    assert args[12] == 128 and args[13].shape == (16, 30) and args[15:] == (False, False)              # sequential, not antithetic
    recorded.clear()
    # the paths
    p.simulate_paths(S, T, R, Q, 1000, 16, 3, scheme="qe")
    p.simulate_paths(S, T, R, Q, 128, 16, 3, **sequential)
    (n0, a0, k0), (n1, a1, k1) = recorded
    assert n0 == "heston_qe_paths" and a0 == (S, T, R, Q, *model, 1000, 16, 3) and k0 == dict(path_major=True)
    assert n1 == "heston_qe_qmc_paths" and a1[:10] == (S, T, R, Q, *model, 128) and a1[10].shape == (32, 30) and a1[12] is False
    assert k1 == dict(path_major=True)
    recorded.clear()
    # the surface: 18 cells, two launches, every answer in its cell; the calibrators pass the scheme on
    strikes, maturities = (80.0, 100.0, 120.0), (0.5, 0.25, 1.0, 0.25, 0.75, 0.0625)
    prices = p.price_surface(S, strikes, maturities, R, Q, "call", 1000, 16, 3, scheme="qe")
    assert [n for n, _a, _k in recorded] == ["heston_qe_surface"] * 2 and [len(a[10]) for _n, a, _k in recorded] == [16, 2]
    assert np.array_equal(prices, np.add.outer(np.array(strikes), np.array([8.0, 4.0, 16.0, 4.0, 12.0, 1.0])))
    recorded.clear()
    objective = hes.calibration_objective(_market(), n_paths=128, n_steps=16, seed=3, path_construction="sequential", scheme="qe")
    objective(model)
    (name, args, _k), = recorded
    assert name == "heston_qe_qmc_surface" and objective.evals == 1 and len(args[10]) == 9


def test_the_default_grid_of_a_qe_calibration_has_16_steps_a_year(recorded):
    hes.calibration_objective(_market(), n_paths=128, path_construction="sequential", scheme="qe")(qe.USUAL)
    hes.calibration_objective(_market(), n_paths=128, path_construction="sequential")(qe.USUAL)
    (n0, a0, _k0), (n1, a1, _k1) = recorded
    assert n0 == "heston_qe_qmc_surface" and a0[13].shape == (32, 30) and sorted(set(a0[11])) == [4, 8, 16]
    assert n1 == "heston_qmc_surface" and a1[13].shape == (128, 30) and sorted(set(a1[11])) == [16, 32, 64]


# ---------------------------------------------------------------------------------------------------- 5. the C ABI ----
def test_the_entry_points_are_declared_bound_and_exported(library):
    from tests.test_abi_cpu import declared_symbols

    for name in QE_NAMES:
        assert name in declared_symbols() and name in _hip.PROTOTYPES and hasattr(library, name)
    assert library.olmc_abi_version() == 6
    assert _hip.STREAM_HESTON_QE == qe.STREAM_HESTON_QE == 0x48514500


def _st(k=16):
    return (_hip.Stats * k)()


def _cells(k=1, step=4):
    return (C.c_double * max(k, 1))(*[100.0] * k), (C.c_int32 * max(k, 1))(*[step] * k)


def _mats():
    return (C.c_double * 8)(), (C.c_double * 8)()


_M = (2.0, 0.04, 0.3, -0.7, 0.04)
_MKT = (100.0, 1.0, 0.05, 0.0)


def _model(**over):
    m = dict(zip(("kappa", "theta", "sigma_v", "rho", "v0"), _M))
    m.update(over)
    return tuple(m.values())


def _surface(model=_M, k=1, step=4, n_steps=4):
    return lambda: (*_MKT, 1, *model, *_cells(k, step), k, 0, 100, n_steps, 1, 0, _st())


def _qmc_surface(model=_M, k=1, construction=0, n_steps=4, bits=30):
    return lambda: (*_MKT, 1, *model, *_cells(k), k, construction, 0, 64, n_steps, *_sobol(2 * n_steps), bits, 0, _st())


def _paths(model=_M):
    return lambda: (*_MKT, *model, 1, 4, 1, 1, *_mats())


def _qmc_paths(model=_M, construction=0):
    return lambda: (*_MKT, *model, construction, 1, 4, *_sobol(8), 30, 1, *_mats())


_BRIDGE = "the QE scheme takes OLMC_QMC_SEQUENTIAL only: its variance draw is a uniform, not a Brownian increment"
_REFUSALS = []
for _make in (_surface, _qmc_surface, _paths, _qmc_paths):
    _name = {_surface: QE_NAMES[0], _qmc_surface: QE_NAMES[1], _paths: QE_NAMES[2], _qmc_paths: QE_NAMES[3]}[_make]
    _REFUSALS += [
        (_name, _make(_model(kappa=0.0)), "kappa must be positive for the QE scheme"),
        (_name, _make(_model(kappa=-1.0)), "kappa must be positive for the QE scheme"),
        (_name, _make(_model(theta=0.0)), "theta must be positive for the QE scheme"),
        (_name, _make(_model(sigma_v=0.0)), "sigma_v must be positive for the QE scheme"),
        (_name, _make(_model(sigma_v=-0.3)), "sigma_v must be positive for the QE scheme"),
        (_name, _make(_model(v0=-1e-9)), "v0 must be non-negative for the QE scheme"),
        (_name, _make(_model(rho=1.5)), "rho must be in [-1, 1]"),
    ]
_REFUSALS += [
    (QE_NAMES[1], _qmc_surface(construction=1), _BRIDGE),
    (QE_NAMES[3], _qmc_paths(construction=1), _BRIDGE),
    (QE_NAMES[1], _qmc_surface(construction=2), "bad construction"),
    (QE_NAMES[3], _qmc_paths(construction=7), "bad construction"),
    (QE_NAMES[0], _surface(k=0), "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    (QE_NAMES[0], _surface(k=17), "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    (QE_NAMES[1], _qmc_surface(k=0), "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    (QE_NAMES[1], _qmc_surface(k=17), "the number of cells must be in [1, OLMC_MAX_BATCH]"),
    (QE_NAMES[0], _surface(step=5), "a cell's step must be in [1, n_steps]"),
    (QE_NAMES[0], _surface(step=0), "a cell's step must be in [1, n_steps]"),
    (QE_NAMES[0], _surface(n_steps=0), "n_steps must be >= 1"),
    (QE_NAMES[1], _qmc_surface(bits=32), "only 30-bit Sobol tables (SciPy's default) are supported"),
    (QE_NAMES[0], lambda: (*_MKT, 1, *_M, None, None, 1, 0, 100, 4, 1, 0, _st()), "null pointer"),
    (QE_NAMES[2], lambda: (*_MKT, *_M, 100, 4, 1, 1, None, None), "null pointer"),
    (QE_NAMES[2], lambda: (*_MKT, *_M, 5 * 10**8, 10, 1, 1, *_mats()), "path matrices would exceed 64 GB"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_the_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    refused(library, getattr(library, name)(*args()), message)
