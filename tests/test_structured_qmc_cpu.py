"""method="qmc" on the autocallable and the cliquet without a device: every refusal comes before the device is touched, "qmc" reaches
the Sobol bindings and "pseudo" the Philox ones with the arguments they always got, a missing GPU is loud, and the C entry points
refuse bad arguments before any device work."""
import math
import os

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests.abi_support import library, no_device, refused, sobol as _sobol, _ST

S, K, T, R, SIG, Q = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0
_BINDINGS = ("lib", "autocallable", "cliquet", "autocallable_qmc", "cliquet_qmc")


def _options():
    return [ol.AutocallableOption(S, K, T, R, SIG, seed=3), ol.CliquetOption(S, K, T, R, SIG, seed=3)]


@pytest.mark.parametrize("kwargs,match", [
    (dict(method="sobol"), "method"),
    (dict(method="QMC"), "method"),
    (dict(method="qmc", path_construction="pca"), "path_construction"),
    (dict(method="pseudo", path_construction="brownian"), "path_construction"),
    (dict(method="qmc", n_steps=21202, path_construction="sequential"), "21201"),
    (dict(method="qmc", n_steps=1025), "1024"),
    (dict(method="qmc", n_steps=1025, path_construction="bridge"), "1024"),
])
def test_refusals_come_before_the_device(no_device, kwargs, match):
    for opt in _options():
        kw = dict(n_paths=100, n_steps=8)
        kw.update(kwargs)
        with pytest.raises(ValueError, match=match):
            opt.price(**kw)


@pytest.fixture
def recorded(monkeypatch):
    """The four bindings record their calls and answer a fixed Stats; the library itself must not be loaded."""
    calls = []

    def recorder(name):
        def call(*a, **k):
            calls.append((name, a, k))
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


def test_qmc_reaches_the_sobol_bindings_and_not_the_philox_ones(recorded):
    from optionslab_amd.monte_carlo import sobol_tables

    auto, cliq = _options()
    for construction, bridge in (("bridge", True), ("sequential", False)):
        del recorded[:]
        got = auto.price(100, 8, observation_freq=2, antithetic=True, method="qmc", path_construction=construction, option_type="call")
        assert isinstance(got, np.float64) and got == 1.25
        assert cliq.price(100, 8, n_periods=4, method="qmc", path_construction=construction, return_error=True) == (1.25, 0.5)
        (name_a, args_a, kw_a), (name_c, args_c, kw_c) = recorded
        assert (name_a, name_c) == ("autocallable_qmc", "cliquet_qmc") and not kw_a and not kw_c
        sv, shift = sobol_tables(8, 3, 100)                                    # the option's seed is the scramble seed
        assert args_a[:11] == (S, T, R, SIG, Q, 1.0, 0.8, 0.10, 0.6, 2, 100) and args_a[13:] == (bridge, True)
        assert args_c[:11] == (S, T, R, SIG, Q, 0.05, -0.05, 0.30, 0.0, 4, 100) and args_c[13:] == (bridge, False)
        for args in (args_a, args_c):
            assert np.array_equal(args[11], sv) and np.array_equal(args[12], shift)


def test_an_autocallable_without_an_observation_date_keeps_its_treatment_on_sobol_paths(recorded):
    _options()[0].price(100, 8, observation_freq=21, method="qmc")
    (name, args, _kw), = recorded
    assert name == "autocallable_qmc" and args[5] == math.inf and args[9] == 8      # one observation, on the last step, at a level no path reaches


@pytest.mark.parametrize("kwargs", [dict(), dict(method="pseudo"), dict(method="pseudo", path_construction="sequential")])
def test_pseudo_and_no_keyword_reach_the_philox_bindings_with_todays_arguments(recorded, kwargs):
    auto, cliq = _options()
    assert auto.price(100, 8, observation_freq=2, option_type="call", **kwargs) == 1.25
    assert cliq.price(100, 8, n_periods=4, antithetic=True, return_error=True, **kwargs) == (1.25, 0.5)
    assert recorded == [
        ("autocallable", (S, T, R, SIG, Q, 1.0, 0.8, 0.10, 0.6, 2, 100, 8, 3, False), {}),
        ("cliquet", (S, T, R, SIG, Q, 0.05, -0.05, 0.30, 0.0, 4, 100, 8, 3, True), {}),
    ]
    del recorded[:]
    auto.price(100, 8, observation_freq=21, **kwargs)
    assert recorded == [("autocallable", (S, T, R, SIG, Q, math.inf, 0.8, 0.10, 0.6, 8, 100, 8, 3, False), {})]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: loud-failure path not reachable")
def test_qmc_without_a_gpu_is_an_acceleration_error():
    for opt in _options():
        for construction in ("bridge", "sequential"):
            with pytest.raises(AccelerationError):
                opt.price(n_paths=64, n_steps=16, method="qmc", path_construction=construction)


def test_the_abi_declares_the_structured_qmc_entry_points():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "olmc.h")) as f:
        header = f.read()
    for name in ("olmc_autocallable_qmc", "olmc_cliquet_qmc"):
        assert name in _hip.PROTOTYPES
        assert f"int {name}(" in header


# ------------------------------------------------------------------------------------------------- the C entry points ----
_MKT = (100.0, 1.0, 0.05, 0.2, 0.0)                               # S T r sigma q
_AUTO = (*_MKT, 1.0, 0.8, 0.10, 0.6)                              # + autocall, coupon level, coupon rate, knock-in
_CLIQ = (*_MKT, 0.05, -0.05, 0.30, 0.0)                           # + local cap, local floor, global cap, global floor
_BRIDGE_CAP = "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"
_BITS = "only 30-bit Sobol tables (SciPy's default) are supported"

# (name, args after the contract: count, construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic, out), message
_REFUSALS = [
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 0, 1, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "observation_freq must be >= 1"),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 9, 0, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "no observation date: observation_freq > n_steps"),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 21, 1, 0, 64, 1025, *_sobol(1025), 30, 0, _ST()), _BRIDGE_CAP),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 2, 1, 0, 64, 8, *_sobol(8), 29, 0, _ST()), _BITS),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 2, 1, 0, 64, 8, None, _sobol(8)[1], 30, 0, _ST()), "null pointer"),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 2, 1, 0, 64, 8, *_sobol(8), 30, 0, None), "null pointer"),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 2, 2, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "bad construction"),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 2, 0, 0, 0, 8, *_sobol(8), 30, 0, _ST()), "n_paths must be >= 1"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 0, 1, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "n_periods must be in [1, n_steps]"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 9, 0, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "n_periods must be in [1, n_steps]"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 12, 1, 0, 64, 1025, *_sobol(1025), 30, 0, _ST()), _BRIDGE_CAP),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 4, 0, 0, 64, 8, *_sobol(8), 29, 0, _ST()), _BITS),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 4, 0, 0, 64, 8, None, _sobol(8)[1], 30, 0, _ST()), "null pointer"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 4, 0, 0, 64, 8, *_sobol(8), 30, 0, None), "null pointer"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 4, -1, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "bad construction"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 4, 0, 0, 64, 0, *_sobol(1), 30, 0, _ST()), "dims must be in [1, 21201]"),
    # two faults at once: the Sobol call's checks come before the product's count
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 0, 2, 0, 64, 8, *_sobol(8), 30, 0, _ST()), "bad construction"),
    ("olmc_autocallable_qmc", lambda: (*_AUTO, 9, 0, 0, 64, 8, *_sobol(8), 32, 0, _ST()), _BITS),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 0, 0, 0, 0, 8, *_sobol(8), 30, 0, _ST()), "n_paths must be >= 1"),
    ("olmc_cliquet_qmc", lambda: (*_CLIQ, 9, 3, 0, 64, 8, *_sobol(8), 30, 0, None), "null pointer"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    """Each refusal answers OLMC_ERR_ARG (1) with its exact message, ahead of any device work (no device is initialised here)."""
    refused(library, getattr(library, name)(*args()), message)


def test_the_refactored_philox_entry_points_still_refuse_as_before(library):
    for name, args, message in [
        ("olmc_autocallable", (*_AUTO, 0, 0, 64, 8, 1, 0, _ST()), "observation_freq must be >= 1"),
        ("olmc_autocallable", (*_AUTO, 9, 0, 64, 8, 1, 0, _ST()), "no observation date: observation_freq > n_steps"),
        ("olmc_cliquet", (*_CLIQ, 9, 0, 64, 8, 1, 0, _ST()), "n_periods must be in [1, n_steps]"),
    ]:
        refused(library, getattr(library, name)(*args), message)
