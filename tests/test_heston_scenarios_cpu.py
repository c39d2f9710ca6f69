"""Host-side checks of the Heston scenario sets and their fused Greeks (no GPU; the library is loaded, never a device): the grouping of
scenarios into recursions (olmc_heston_scenario_layout), the refusals that come before the device in Python and at the C ABI, the greedy
cut of a scenario list into launches, and the adapter's conventions."""
import ctypes as C

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from optionslab_amd import heston as hes
from optionslab_amd.greeks import fd_steps
from tests.abi_support import library, no_library, _out17 as _out, refused, sobol as _sobol

S, K, T, R, Q = 100.0, 100.0, 1.0, 0.05, 0.02
MODEL = (2.0, 0.04, 0.3, -0.7, 0.04)                      # kappa theta sigma_v rho v0


def scenario(S_=S, K_=K, T_=T, r_=R, q_=Q, call=True, model=MODEL, **over):
    m = dict(zip(("kappa", "theta", "sigma_v", "rho", "v0"), model))
    m.update(over)
    return (S_, K_, T_, r_, q_, call, m["kappa"], m["theta"], m["sigma_v"], m["rho"], m["v0"])


def greeks_scenarios(sigma=0.2, T_=T, second=True):
    """The contracts of compute_greeks_unified in its call order, sigma -> v0 = sigma^2."""
    h_S, h_v, h_r, h_T = fd_steps(S)
    has_T = T_ > h_T
    bumps = [(S, T_, R, sigma), (S + h_S, T_, R, sigma), (S - h_S, T_, R, sigma), (S, T_, R, sigma + h_v), (S, T_, R, sigma - h_v)]
    if has_T:
        bumps.append((S, T_ - h_T, R, sigma))
    bumps += [(S, T_, R + h_r, sigma), (S, T_, R - h_r, sigma)]
    if second:
        bumps += [(S + h_S, T_, R, sigma + h_v), (S + h_S, T_, R, sigma - h_v), (S - h_S, T_, R, sigma + h_v), (S - h_S, T_, R, sigma - h_v)]
        if has_T:
            bumps += [(S + h_S, T_ - h_T, R, sigma), (S - h_S, T_ - h_T, R, sigma)]
    return [scenario(S_=s, T_=t, r_=r, v0=v * v) for s, t, r, v in bumps]


# ------------------------------------------------------------------------------------------------------ the layout ----
def test_the_fourteen_greeks_contracts_are_four_recursions(library):
    sc = greeks_scenarios()
    assert len(sc) == 14
    n_rec, group = _hip.heston_scenario_layout(sc)
    assert n_rec == 4
    #               mid S+ S- v+ v- T- r+ r- uu ud du dd ut dt
    assert group == [0, 0, 0, 1, 2, 3, 0, 0, 1, 2, 1, 2, 3, 3]


def test_first_order_and_short_maturities(library):
    sc = greeks_scenarios(second=False)
    assert len(sc) == 8
    assert _hip.heston_scenario_layout(sc) == (4, [0, 0, 0, 1, 2, 3, 0, 0])
    sc = greeks_scenarios(T_=1 / 400)                                                # T <= h_T: no T bump
    assert len(sc) == 11
    assert _hip.heston_scenario_layout(sc) == (3, [0, 0, 0, 1, 2, 0, 0, 1, 2, 1, 2])
    sc = greeks_scenarios(T_=1 / 400, second=False)
    assert _hip.heston_scenario_layout(sc) == (3, [0, 0, 0, 1, 2, 0, 0])


def test_recursions_are_numbered_by_first_appearance(library):
    keys = [dict(T_=0.5), dict(kappa=3.0), dict(), dict(theta=0.05), dict(sigma_v=0.4), dict(rho=0.1)]      # six recursions
    order = [3, 0, 3, 5, 1, 0, 2, 2, 4, 5, 1, 3, 0, 4, 2, 5]
    sc = [scenario(S_=90.0 + i, K_=110.0 - i, r_=0.01 * (i % 3), call=bool(i % 2), **keys[g]) for i, g in enumerate(order)]
    n_rec, group = _hip.heston_scenario_layout(sc)
    first = []
    for g in order:
        if g not in first:
            first.append(g)
    assert n_rec == 6 and first == [3, 0, 5, 1, 2, 4]
    assert group == [first.index(g) for g in order]
    assert _hip.heston_scenario_layout([sc[0]]) == (1, [0])


def test_seven_recursions_are_refused(library):
    sc = [scenario(v0=0.01 * (i + 1)) for i in range(7)]
    arr, k = _hip._scenarios(sc)
    n_rec, group = C.c_int32(-1), (C.c_int32 * 7)()
    assert library.olmc_heston_scenario_layout(arr, k, C.byref(n_rec), group) == 1
    assert b"OLMC_HESTON_MAX_RECURSIONS" in library.olmc_last_error()
    assert _hip.heston_scenario_layout(sc[:6]) == (6, list(range(6)))
    for bad_k in (0, 17):
        assert library.olmc_heston_scenario_layout(arr, bad_k, C.byref(n_rec), group) == 1
    assert library.olmc_heston_scenario_layout(None, 1, C.byref(n_rec), group) == 1
    assert library.olmc_heston_scenario_layout(arr, 1, None, group) == 1
    assert library.olmc_heston_scenario_layout(arr, 1, C.byref(n_rec), None) == 1


def test_the_grouping_key_is_the_doubles_themselves(library):
    assert 0.2**2 != 0.04
    assert _hip.heston_scenario_layout([scenario(v0=0.04), scenario(v0=0.2**2), scenario(v0=0.04)]) == (2, [0, 1, 0])
    assert _hip.heston_scenario_layout([scenario(T_=0.3), scenario(T_=0.1 + 0.2)]) == (2, [0, 1])
    # spot, strike, rates and call / put never split a recursion
    assert _hip.heston_scenario_layout([scenario(), scenario(S_=90.0, K_=80.0, r_=0.0, q_=0.1, call=False)]) == (1, [0, 0])
    for name in ("kappa", "theta", "sigma_v", "rho", "v0"):
        assert _hip.heston_scenario_layout([scenario(), scenario(**{name: 0.5})]) == (2, [0, 1]), name


# ---------------------------------------------------------------------------------------------- the Python refusals ----
GOOD = dict(S=S, K=K, T=T, r=R)


@pytest.mark.parametrize("scenarios,kw,match", [
    ([], dict(), "empty"),
    ([dict(S=S, K=K, r=R)], dict(), "lacks"),
    ([GOOD, dict(S=S, T=T, r=R)], dict(), "scenario 1 lacks"),
    ([dict(GOOD, T=0.0)], dict(), "T must be > 0"),
    ([dict(GOOD, T=-1.0)], dict(), "T must be > 0"),
    ([dict(GOOD, rho=1.5)], dict(), "rho"),
    ([dict(GOOD, vol=0.2)], dict(), "unknown"),
    ([GOOD], dict(scheme="qe"), "Euler"),
    ([GOOD], dict(scheme="milstein"), "scheme"),
    ([GOOD], dict(n_paths=0), ">= 1"),
    ([GOOD], dict(n_steps=0), ">= 1"),
    ([GOOD], dict(method="sobol"), "method"),
    ([GOOD], dict(method="qmc", path_construction="pca"), "path_construction"),
    ([GOOD], dict(method="qmc", n_steps=2048), "1024"),
    ([GOOD], dict(method="qmc", path_construction="sequential", n_steps=10601), "10600"),
    ([GOOD], dict(method="qmc", n_paths=(1 << 30) + 1), "2\\*\\*30"),
])
def test_price_scenarios_refuses_before_the_device(no_library, scenarios, kw, match):
    with pytest.raises(ValueError, match=match):
        ol.HestonPricer(*MODEL).price_scenarios(scenarios, **{"n_paths": 100, "n_steps": 8, "seed": 1, **kw})


@pytest.mark.parametrize("kw,match", [
    (dict(scheme="qe"), "Euler"),
    (dict(n_paths=0), ">= 1"),
    (dict(n_steps=0), ">= 1"),
    (dict(method="sobol"), "method"),
    (dict(method="qmc", path_construction="pca"), "path_construction"),
    (dict(method="qmc", n_steps=2048), "1024"),
])
def test_the_adapter_refuses_before_the_device(no_library, kw, match):
    p = ol.HestonPricer(*MODEL)
    with pytest.raises(ValueError, match=match):
        ol.HestonMCAdapter(p, **{"n_paths": 100, "n_steps": 8, "seed": 1, **kw})
    with pytest.raises(ValueError, match=match):
        ol.greeks_heston_monte_carlo(p, S, K, T, R, **{"n_paths": 100, "n_steps": 8, "seed": 1, **kw})


def test_the_adapter_reaches_the_device_only_to_price(no_library):
    p = ol.HestonPricer(*MODEL)
    adapter = ol.HestonMCAdapter(p, 100, 8)
    assert isinstance(adapter.seed, int) and adapter._can_fuse({}) and not adapter._can_fuse({"seed": 1})
    again = ol.HestonMCAdapter(p, 100, 8, seed=5, method="qmc")
    assert again.seed == 5 and again._qmc is not None
    for a in (adapter, again):
        with pytest.raises(AssertionError, match="touched"):
            a.price(S, K, T, R, 0.25, "call", Q)
        with pytest.raises(ol.GreeksError, match="touched"):
            ol.compute_greeks_unified(a, S, K, T, R, 0.2, "call", Q)
    assert p.v0 == 0.04


def test_the_new_names_are_exported():
    for name in ("HestonMCAdapter", "greeks_heston_monte_carlo"):
        assert name in ol.__all__ and hasattr(ol, name)
    assert hasattr(ol.HestonPricer, "price_scenarios")
    for name in ("heston_scenario_layout", "heston_scenarios", "heston_qmc_scenarios", "heston_greeks_fd", "heston_qmc_greeks_fd"):
        assert callable(getattr(_hip, name))


# ------------------------------------------------------------------------------------------- the C ABI's refusals ----
def _sc(*scenarios):
    return _hip._scenarios(list(scenarios) or [scenario()])


_SEVEN = [scenario(v0=0.01 * (i + 1)) for i in range(7)]
_GREEKS = (S, K, T, R, 0.2, Q, 1, 2.0, 0.04, 0.3)                                   # ... rho follows
_REFUSALS = [
    ("olmc_heston_scenarios", lambda: (None, 1, 0, 100, 4, 1, 0, _out()), "null pointer"),
    ("olmc_heston_scenarios", lambda: (*_sc(), 0, 100, 4, 1, 0, None), "null pointer"),
    ("olmc_heston_scenarios", lambda: (_sc()[0], 0, 0, 100, 4, 1, 0, _out()), "the number of scenarios must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_heston_scenarios", lambda: (_sc()[0], 17, 0, 100, 4, 1, 0, _out()), "the number of scenarios must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_heston_scenarios", lambda: (*_sc(*_SEVEN), 0, 100, 4, 1, 0, _out()),
     "more than OLMC_HESTON_MAX_RECURSIONS distinct (T, kappa, theta, sigma_v, rho, v0)"),
    ("olmc_heston_scenarios", lambda: (*_sc(scenario(), scenario(T_=0.0)), 0, 100, 4, 1, 0, _out()), "T must be > 0 in every scenario"),
    ("olmc_heston_scenarios", lambda: (*_sc(scenario(T_=-1.0)), 0, 100, 4, 1, 0, _out()), "T must be > 0 in every scenario"),
    ("olmc_heston_scenarios", lambda: (*_sc(scenario(), scenario(rho=1.5)), 0, 100, 4, 1, 0, _out()), "rho must be in [-1, 1]"),
    ("olmc_heston_scenarios", lambda: (*_sc(), 0, 0, 4, 1, 0, _out()), "n_paths must be >= 1"),
    ("olmc_heston_scenarios", lambda: (*_sc(), 0, 100, 0, 1, 0, _out()), "n_steps must be >= 1"),
    ("olmc_heston_scenarios", lambda: (*_sc(), -1, 100, 4, 1, 0, _out()), "path_offset must be >= 0"),
    ("olmc_heston_qmc_scenarios", lambda: (None, 1, 0, 0, 64, 4, *_sobol(8), 30, 0, _out()), "null pointer"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 0, 0, 64, 4, *_sobol(8), 30, 0, None), "null pointer"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 0, 0, 64, 4, None, None, 30, 0, _out()), "null pointer"),
    ("olmc_heston_qmc_scenarios", lambda: (_sc()[0], 17, 0, 0, 64, 4, *_sobol(8), 30, 0, _out()),
     "the number of scenarios must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(*_SEVEN), 0, 0, 64, 4, *_sobol(8), 30, 0, _out()),
     "more than OLMC_HESTON_MAX_RECURSIONS distinct (T, kappa, theta, sigma_v, rho, v0)"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(scenario(T_=0.0)), 0, 0, 64, 4, *_sobol(8), 30, 0, _out()), "T must be > 0 in every scenario"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(scenario(rho=-1.5)), 0, 0, 64, 4, *_sobol(8), 30, 0, _out()), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 2, 0, 64, 4, *_sobol(8), 30, 0, _out()), "bad construction"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 1, 0, 64, 1025, *_sobol(1), 30, 0, _out()),
     "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 0, 0, 64, 0, *_sobol(1), 30, 0, _out()),
     "n_steps must be in [1, 10600]: a step takes two of the 21201 Sobol dimensions"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 0, 0, 64, 4, *_sobol(8), 32, 0, _out()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 0, 0, 0, 4, *_sobol(8), 30, 0, _out()), "n_paths must be >= 1"),
    ("olmc_heston_greeks_fd", lambda: (*_GREEKS, -0.7, 100, 4, 1, 0, 1, None, None), "null pointer"),
    ("olmc_heston_greeks_fd", lambda: (S, K, 0.0, R, 0.2, Q, 1, 2.0, 0.04, 0.3, -0.7, 100, 4, 1, 0, 1, (C.c_double * 9)(), None), "T must be > 0"),
    ("olmc_heston_greeks_fd", lambda: (*_GREEKS, 1.5, 100, 4, 1, 0, 1, (C.c_double * 9)(), None), "rho must be in [-1, 1]"),
    ("olmc_heston_greeks_fd", lambda: (*_GREEKS, -0.7, 0, 4, 1, 0, 1, (C.c_double * 9)(), None), "n_paths must be >= 1"),
    ("olmc_heston_greeks_fd", lambda: (*_GREEKS, -0.7, 100, 0, 1, 0, 1, (C.c_double * 9)(), None), "n_steps must be >= 1"),
    ("olmc_heston_qmc_greeks_fd", lambda: (*_GREEKS, -0.7, 0, 64, 4, *_sobol(8), 30, 0, 1, None, None), "null pointer"),
    ("olmc_heston_qmc_greeks_fd", lambda: (*_GREEKS, -0.7, 0, 64, 4, None, None, 30, 0, 1, (C.c_double * 9)(), None), "null pointer"),
    ("olmc_heston_qmc_greeks_fd", lambda: (*_GREEKS, -0.7, 3, 64, 4, *_sobol(8), 30, 0, 1, (C.c_double * 9)(), None), "bad construction"),
    ("olmc_heston_qmc_greeks_fd", lambda: (*_GREEKS, 1.5, 0, 64, 4, *_sobol(8), 30, 0, 1, (C.c_double * 9)(), None), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc_greeks_fd", lambda: (*_GREEKS, -0.7, 1, 64, 1025, *_sobol(1), 30, 0, 1, (C.c_double * 9)(), None),
     "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"),
    # two faults at once: the scenario list before the Sobol call
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(scenario(rho=-1.5)), 2, 0, 64, 4, *_sobol(8), 30, 0, _out()), "rho must be in [-1, 1]"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(*_SEVEN), 2, 0, 64, 4, *_sobol(8), 32, 0, _out()),
     "more than OLMC_HESTON_MAX_RECURSIONS distinct (T, kappa, theta, sigma_v, rho, v0)"),
    ("olmc_heston_qmc_scenarios", lambda: (*_sc(), 2, 0, 64, 4, *_sobol(8), 32, 0, _out()), "bad construction"),
    ("olmc_heston_qmc_greeks_fd", lambda: (S, K, 0.0, R, 0.2, Q, 1, 2.0, 0.04, 0.3, -0.7, 3, 64, 4, *_sobol(8), 30, 0, 1, (C.c_double * 9)(), None),
     "T must be > 0"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    """Each refusal answers OLMC_ERR_ARG (1) with its exact message, ahead of any device work (no device is initialised here)."""
    refused(library, getattr(library, name)(*args()), message)


def test_the_bindings_check_the_tables(no_library):
    sv, shift = np.ones((7, 30), np.uint32), np.zeros(7, np.uint32)
    with pytest.raises(ValueError, match="even"):
        _hip.heston_qmc_scenarios([scenario()], 64, sv, shift)
    with pytest.raises(ValueError, match="even"):
        _hip.heston_qmc_greeks_fd(S, K, T, R, 0.2, Q, True, *MODEL[:4], 64, sv, shift, True, False, True)


# ------------------------------------------------------------------------------------------------------ the split ----
def test_the_greedy_split_of_twenty_scenarios_and_nine_recursions():
    """Recursions a .. i.  The first launch ends where the seventh recursion (g) would enter, the second where its 17th scenario would;
    hand-written."""
    keys = list("aabbccddeeffgabghhia")
    assert len(keys) == 20 and len(set(keys)) == 9
    assert hes._scenario_launches(keys) == [list(range(0, 12)), list(range(12, 20))]
    # a launch is cut at 16 scenarios even when the recursions would fit
    assert hes._scenario_launches(["a"] * 35) == [list(range(0, 16)), list(range(16, 32)), [32, 33, 34]]
    # ... and at the seventh recursion even when it is short; a recursion seen again after the cut counts anew
    keys = list("abcdefgabcdefhh")
    assert hes._scenario_launches(keys) == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [12, 13, 14]]
    assert hes._scenario_launches([]) == [] and hes._scenario_launches(["x"]) == [[0]]
    assert hes._scenario_launches(list("abcdef") * 3) == [list(range(16)), [16, 17]]


def test_the_split_keys_compare_the_doubles_bit_for_bit():
    assert hes._recursion_key(T, *MODEL) == hes._recursion_key(1.0, 2.0, 0.04, 0.3, -0.7, 0.04)
    assert hes._recursion_key(T, *MODEL[:4], 0.2**2) != hes._recursion_key(T, *MODEL)
    assert hes._recursion_key(0.1 + 0.2, *MODEL) != hes._recursion_key(0.3, *MODEL)


def test_price_scenarios_sends_the_split_with_one_seed(monkeypatch):
    """20 scenarios of 9 recursions reach the binding as the two launches of the hand-written split, with the defaults filled in and
    one seed (seed=None draws it once)."""
    calls = []

    def fake(scenarios, n_paths, n_steps, seed, antithetic=False, path_offset=0):
        calls.append((list(scenarios), n_paths, n_steps, seed, antithetic))
        out = []
        for sc in scenarios:
            st = _hip.Stats()
            st.price, st.std_error = sc[1], sc[10]                                   # the strike and v0 come back: the order is checked below
            out.append(st)
        return out

    monkeypatch.setattr(_hip, "heston_scenarios", fake)
    v0s = dict(zip("abcdefghi", (0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09)))
    scenarios = [dict(S=S, K=50.0 + i, T=T, r=R, v0=v0s[c]) for i, c in enumerate("aabbccddeeffgabghhia")]
    scenarios[3].update(q=0.03, option_type="put")
    p = ol.HestonPricer(*MODEL)
    prices, errors = p.price_scenarios(scenarios, 100, 8, None, True, return_error=True)
    assert [len(c[0]) for c in calls] == [12, 8]
    assert calls[0][3] == calls[1][3] and all(c[1:3] == (100, 8) and c[4] is True for c in calls)
    assert list(prices) == [50.0 + i for i in range(20)] and list(errors) == [v0s[c] for c in "aabbccddeeffgabghhia"]
    assert prices.dtype == np.float64 and prices.shape == (20,)
    first = calls[0][0]
    assert first[0] == (S, 50.0, T, R, 0.0, True, 2.0, 0.04, 0.3, -0.7, 0.01)
    assert first[3] == (S, 53.0, T, R, 0.03, False, 2.0, 0.04, 0.3, -0.7, 0.02)
    only = p.price_scenarios(scenarios[:1], 100, 8, 3)
    assert only.shape == (1,) and calls[-1][3] == 3
