"""method="qmc" on HestonPricer without a device: every refusal comes before the device is touched, "qmc" reaches the Sobol bindings
with tables of 2 n dimensions, "pseudo" and the default reach the Philox ones with the arguments they always got, a missing GPU is
loud, and the C entry points refuse bad arguments before any device work."""
import os

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests.abi_support import library, no_device, _out, refused, sobol as _sobol, _ST

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.01
MODEL = (2.0, 0.04, 0.3, -0.7, 0.04)                      # kappa theta sigma_v rho v0
_BINDINGS = ("lib", "heston", "heston_paths", "heston_qmc", "heston_qmc_paths")


def _pricer():
    return ol.HestonPricer(*MODEL)


def _calls(pricer):
    """The two public calls as functions of their keywords (n_paths, n_steps and the rest)."""
    return [lambda **kw: pricer.price_monte_carlo(S, K, T, R, Q, "call", **kw), lambda **kw: pricer.simulate_paths(S, T, R, Q, **kw)]


@pytest.mark.parametrize("kwargs,match", [
    (dict(method="sobol"), "method"),
    (dict(method="QMC"), "method"),
    (dict(method="qmc", path_construction="pca"), "path_construction"),
    (dict(method="pseudo", path_construction="brownian"), "path_construction"),
    (dict(method="qmc", n_steps=10601, path_construction="sequential"), "10600"),
    (dict(method="qmc", n_steps=21201, path_construction="sequential"), "10600"),
    (dict(method="qmc", n_steps=1025), "1024"),
    (dict(method="qmc", n_steps=1025, path_construction="bridge"), "1024"),
    (dict(method="qmc", n_paths=(1 << 30) + 1), r"2\*\*30"),
    (dict(method="qmc", n_paths=0), "n_paths"),
    (dict(method="qmc", n_steps=0), "n_steps"),
])
def test_refusals_come_before_the_device(no_device, kwargs, match):
    for call in _calls(_pricer()):
        kw = dict(n_paths=100, n_steps=8)
        kw.update(kwargs)
        with pytest.raises(ValueError, match=match):
            call(**kw)


def test_the_new_keywords_are_keyword_only(no_device):
    p = _pricer()
    with pytest.raises(TypeError):
        p.price_monte_carlo(S, K, T, R, Q, "call", 100, 8, 3, False, False, "qmc")
    with pytest.raises(TypeError):
        p.simulate_paths(S, T, R, Q, 100, 8, 3, "qmc")


@pytest.fixture
def recorded(monkeypatch):
    """The four bindings record their calls and answer fixed values; the library itself must not be loaded."""
    calls = []

    def recorder(name):
        def call(*a, **k):
            calls.append((name, a, k))
            if name.endswith("paths"):
                return np.zeros((1, 1)), np.ones((1, 1))
            st = _hip.Stats()
            st.price, st.std_error = 1.25, 0.5
            return st
        return call

    def touched(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_hip, "lib", touched)
    for name in _BINDINGS[1:]:
        monkeypatch.setattr(_hip, name, recorder(name), raising=False)
    return calls


def test_qmc_reaches_the_sobol_bindings_with_tables_of_two_dimensions_per_step(recorded):
    from optionslab_amd.monte_carlo import sobol_tables

    p = _pricer()
    sv, shift = sobol_tables(16, 3, 100)                                    # d = 2 n; the seed is the scramble seed
    assert sv.shape == (16, 30) and shift.shape == (16,)
    for construction, bridge in (("bridge", True), ("sequential", False)):
        del recorded[:]
        got = p.price_monte_carlo(S, K, T, R, Q, "put", 100, 8, 3, True, method="qmc", path_construction=construction)
        assert isinstance(got, np.float64) and got == 1.25
        assert p.price_monte_carlo(S, K, T, R, Q, "call", 100, 8, seed=3, return_error=True, method="qmc",
                                   path_construction=construction) == (1.25, 0.5)
        spot, var = p.simulate_paths(S, T, R, Q, 100, 8, 3, method="qmc", path_construction=construction)
        assert spot.shape == var.shape == (1, 1)
        (n1, a1, k1), (n2, a2, k2), (n3, a3, k3) = recorded
        assert (n1, n2, n3) == ("heston_qmc", "heston_qmc", "heston_qmc_paths") and not k1 and not k2
        assert a1[:12] == (S, K, T, R, Q, False, *MODEL, 100) and a1[14:] == (bridge, True)
        assert a2[:12] == (S, K, T, R, Q, True, *MODEL, 100) and a2[14:] == (bridge, False)
        assert a3[:10] == (S, T, R, Q, *MODEL, 100) and a3[12:] == (bridge,) and k3 == dict(path_major=True)
        for tables in (a1[12:14], a2[12:14], a3[10:12]):
            assert np.array_equal(tables[0], sv) and np.array_equal(tables[1], shift)


def test_the_default_construction_is_the_bridge_and_no_seed_draws_a_scramble(recorded):
    p = _pricer()
    p.price_monte_carlo(S, K, T, R, Q, "call", 100, 8, seed=3, method="qmc")
    p.price_monte_carlo(S, K, T, R, Q, "call", 100, 8, method="qmc")
    p.price_monte_carlo(S, K, T, R, Q, "call", 100, 8, method="qmc")
    (_, a, _k), (_, b, _k2), (_, c, _k3) = recorded
    assert a[14] is True and b[14] is True
    assert b[12].shape == (16, 30) and not np.array_equal(b[13], c[13])             # two fresh scrambles


@pytest.mark.parametrize("kwargs", [dict(), dict(method="pseudo"), dict(method="pseudo", path_construction="sequential")])
def test_pseudo_and_no_keyword_reach_the_philox_bindings_with_todays_arguments(recorded, kwargs):
    p = _pricer()
    assert p.price_monte_carlo(S, K, T, R, Q, "call", 100, 8, 3, **kwargs) == 1.25
    assert p.price_monte_carlo(S, K, T, R, Q, "put", 100, 8, 3, True, True, **kwargs) == (1.25, 0.5)
    p.simulate_paths(S, T, R, Q, 100, 8, 3, **kwargs)
    assert recorded == [
        ("heston", (S, K, T, R, Q, True, *MODEL, 100, 8, 3, False), {}),
        ("heston", (S, K, T, R, Q, False, *MODEL, 100, 8, 3, True), {}),
        ("heston_paths", (S, T, R, Q, *MODEL, 100, 8, 3), dict(path_major=True)),
    ]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: loud-failure path not reachable")
def test_qmc_without_a_gpu_is_an_acceleration_error():
    for call in _calls(_pricer()):
        for construction in ("bridge", "sequential"):
            with pytest.raises(AccelerationError):
                call(n_paths=64, n_steps=16, seed=1, method="qmc", path_construction=construction)


def test_the_abi_declares_the_heston_qmc_entry_points():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "olmc.h")) as f:
        header = f.read()
    for name in ("olmc_heston_qmc", "olmc_heston_qmc_paths"):
        assert name in _hip.PROTOTYPES
        assert f"int {name}(" in header
    assert "#define OLMC_ABI_VERSION 6 " in header


def test_the_bindings_refuse_tables_with_an_odd_number_of_dimensions(monkeypatch):
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was loaded"))
    sv, shift = np.ones((7, 30), np.uint32), np.zeros(7, np.uint32)
    with pytest.raises(ValueError, match="even"):
        _hip.heston_qmc(S, K, T, R, Q, True, *MODEL, 64, sv, shift)
    with pytest.raises(ValueError, match="even"):
        _hip.heston_qmc_paths(S, T, R, Q, *MODEL, 64, sv, shift)


# ------------------------------------------------------------------------------------------------- the C entry points ----
_PRICE = (S, K, T, R, Q, 1, *MODEL)                               # S K T r q is_call kappa theta sigma_v rho v0
_PATHS = (S, T, R, Q, *MODEL)
_BAD_RHO = (S, K, T, R, Q, 1, 2.0, 0.04, 0.3, -1.5, 0.04)
_BRIDGE_CAP = "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"
_BITS = "only 30-bit Sobol tables (SciPy's default) are supported"
_STEPS = "n_steps must be in [1, 10600]: a step takes two of the 21201 Sobol dimensions"

# olmc_heston_qmc: contract, construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic, out
# olmc_heston_qmc_paths: contract, construction, n_points, n_steps, sv, shift, bits, path_major, spot, var
_REFUSALS = [
    ("olmc_heston_qmc", lambda: (*_PRICE, 1, 0, 64, 1025, *_sobol(2), 30, 0, _ST()), _BRIDGE_CAP),
    ("olmc_heston_qmc", lambda: (*_PRICE, 0, 0, 64, 10601, *_sobol(2), 30, 0, _ST()), _STEPS),
    ("olmc_heston_qmc", lambda: (*_PRICE, 0, 0, 64, 0, *_sobol(2), 30, 0, _ST()), _STEPS),
    ("olmc_heston_qmc", lambda: (*_PRICE, 1, 0, 64, 8, *_sobol(16), 29, 0, _ST()), _BITS),
    ("olmc_heston_qmc", lambda: (*_PRICE, 1, 0, 64, 8, None, _sobol(16)[1], 30, 0, _ST()), "null pointer"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 1, 0, 64, 8, _sobol(16)[0], None, 30, 0, _ST()), "null pointer"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 1, 0, 64, 8, *_sobol(16), 30, 0, None), "null pointer"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 2, 0, 64, 8, *_sobol(16), 30, 0, _ST()), "bad construction"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 0, 0, 0, 8, *_sobol(16), 30, 0, _ST()), "n_paths must be >= 1"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 0, 1, 1 << 30, 8, *_sobol(16), 30, 0, _ST()), "at most 2**30 Sobol points"),
    ("olmc_heston_qmc", lambda: (*_BAD_RHO, 0, 0, 64, 8, *_sobol(16), 30, 0, _ST()), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 1, 4, 1025, *_sobol(2), 30, 1, _out(1, 1), _out(1, 1)), _BRIDGE_CAP),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 4, 10601, *_sobol(2), 30, 1, _out(1, 1), _out(1, 1)), _STEPS),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 4, 8, *_sobol(16), 31, 1, _out(4, 8), _out(4, 8)), _BITS),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 4, 8, *_sobol(16), 30, 1, None, _out(4, 8)), "null pointer"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 4, 8, *_sobol(16), 30, 1, _out(4, 8), None), "null pointer"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 4, 8, None, _sobol(16)[1], 30, 1, _out(4, 8), _out(4, 8)), "null pointer"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, -1, 4, 8, *_sobol(16), 30, 1, _out(4, 8), _out(4, 8)), "bad construction"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 0, 8, *_sobol(16), 30, 1, _out(1, 8), _out(1, 8)), "n_paths must be >= 1"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 1 << 30, 10600, *_sobol(2), 30, 1, _out(1, 1), _out(1, 1)),
     "path matrix would exceed 64 GB: lower n_paths or n_steps"),
    ("olmc_heston_qmc_paths", lambda: (S, T, R, Q, 2.0, 0.04, 0.3, 1.01, 0.04, 0, 4, 8, *_sobol(16), 30, 1, _out(4, 8), _out(4, 8)),
     "rho must be in [-1, 1]"),
    # two faults at once: the model before the Sobol call, and inside it construction, bridge cap, steps, tables, bits, points, matrix
    ("olmc_heston_qmc", lambda: (*_BAD_RHO, 2, 0, 64, 8, *_sobol(16), 30, 0, _ST()), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 0, 0, 64, 10601, *_sobol(2), 32, 0, _ST()), _STEPS),
    ("olmc_heston_qmc", lambda: (*_PRICE, 2, 0, 64, 10601, *_sobol(2), 30, 0, _ST()), "bad construction"),
    ("olmc_heston_qmc", lambda: (*_PRICE, 0, 0, 0, 8, *_sobol(16), 32, 0, _ST()), _BITS),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 2, 1 << 30, 10600, *_sobol(2), 30, 1, _out(1, 1), _out(1, 1)), "bad construction"),
    ("olmc_heston_qmc_paths", lambda: (*_PATHS, 0, 1 << 30, 10600, *_sobol(2), 29, 1, _out(1, 1), _out(1, 1)), _BITS),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    """Each refusal answers OLMC_ERR_ARG (1) with its exact message, ahead of any device work (no device is initialised here)."""
    refused(library, getattr(library, name)(*args()), message)


def test_the_philox_heston_entry_points_still_refuse_as_before(library):
    refused(library, library.olmc_heston(*_BAD_RHO, 0, 64, 8, 1, 0, _ST()), "rho must be in [-1, 1]")
    refused(library, library.olmc_heston(*_PRICE, 0, 64, 8, 1, 0, None), "null pointer")
    refused(library, library.olmc_heston_paths(S, T, R, Q, 2.0, 0.04, 0.3, -1.5, 0.04, 4, 8, 1, 1, _out(4, 8), _out(4, 8)), "rho must be in [-1, 1]")
    assert library.olmc_abi_version() == 6
