"""CPU checks of the jump-diffusion scenario sets and their fused Greeks (include/olmc_jump_scenarios.h, price_scenarios, JumpMCAdapter).
No GPU: the library is loaded, never a device.

  ABI        the header's declarations = the library's oljs_* exports = _hip.JS_PROTOTYPES; the header is plain C; oljs_scenario's layout
             is the ctypes structure's; the other families' tables and the ABI version stay as they are.
  layout     oljs_layout: the Greeks set is two groups, a mixed set's groups come in order of first appearance, the key is the doubles
             themselves, a Merton a3 never splits.
  fold       the NumPy oracle of the folded definition (tests/jump_scenario_oracle.py) against the last column of the interleaved sum of
             oracle/philox_oracle.py's jump_paths, for every set and shape tests/test_gpu_jump_scenarios.py ties the device to, at that
             test's bar: this is what licenses that bar there.
  refusals   every message of the C ABI, before any device work; Python's ValueErrors before the library is loaded.
  sanitizers the host fold compiled on its own by g++ with AddressSanitizer + UBSan and run as a program (tests/jump_scenario_harness.cpp).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import jump_scenario_cases as jc
from tests import jump_scenario_oracle as jo
from tests.abi_support import _out9, _out17, assert_header_matches, library, no_library, refused
from tests.test_jump_payoffs_cpu import c_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc_jump_scenarios.h")
NAMES = ["oljs_greeks_fd", "oljs_layout", "oljs_scenarios"]
TIE = dict(rel=1e-10, abs=1e-12)
S, K, T, R, Q, SIGMA = jc.S, jc.K, jc.T, jc.R, jc.Q, jc.SIGMA
scenario = jc.scenario


# --------------------------------------------------------------------------------------------------------- the ABI ----
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_header.c"
    src.write_text('#include "olmc_jump_scenarios.h"\n'
                   "int use(const oljs_scenario* sc, const oljd_model* m, int32_t* g, double* out9, olmc_stats* out) {\n"
                   "    return oljs_layout(sc, 2, g, g + 1) + oljs_scenarios(sc, 2, 0, 1000, 8, 1, 0, out)\n"
                   "        + oljs_greeks_fd(100, 100, 1, 0.05, 0.2, 0, 1, m, 1000, 8, 1, 0, 1, out9, out); }\n")
    subprocess.run([*c_compiler(), "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "oljs_", _hip.JS_PROTOTYPES, NAMES)
    for other in (_hip.PROTOTYPES, _hip.LV_PROTOTYPES, _hip.LVQ_PROTOTYPES, _hip.JD_PROTOTYPES):
        assert not any(name.startswith("oljs_") for name in other)
    for name in ("jd_scenario_layout", "jd_scenarios", "jd_greeks_fd"):
        assert callable(getattr(_hip, name))


def test_the_scenario_struct_has_the_headers_layout(tmp_path):
    fields = ("S", "K", "T", "r", "sigma", "q", "is_call", "model", "lambda_j", "a1", "a2", "a3")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "olmc_jump_scenarios.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu", sizeof(oljs_scenario));\n'
                   + "".join(f'    printf(" %zu", offsetof(oljs_scenario, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([*c_compiler(), "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_hip.JsScenario)] + [getattr(_hip.JsScenario, f).offset for f in fields]
    assert got == [88, 0, 8, 16, 24, 32, 40, 48, 52, 56, 64, 72, 80]
    arr, k = _hip._jd_scenarios([scenario(model=jc.KOU, call=False)])
    s = arr[0]
    assert k == 1 and (s.S, s.K, s.T, s.r, s.sigma, s.q, s.is_call, s.model, s.lambda_j, s.a1, s.a2, s.a3) == (S, K, T, R, SIGMA, Q, 0, 1, 60.0, 0.6, 25.0, 20.0)


# ------------------------------------------------------------------------------------------------------ the layout ----
@pytest.mark.parametrize("model", list(jc.MODELS))
def test_the_greeks_contracts_are_two_jump_groups(library, model):
    m = jc.MODELS[model]
    sc = jc.greeks_set(m)
    assert len(sc) == 14
    #                                               mid S+ S- v+ v- T- r+ r- uu ud du dd ut dt
    assert _hip.jd_scenario_layout(sc) == (2, [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1])
    assert _hip.jd_scenario_layout(jc.greeks_set(m, second=False)) == (2, [0, 0, 0, 0, 0, 1, 0, 0])
    assert _hip.jd_scenario_layout(jc.greeks_set(m, T_=1 / 400)) == (1, [0] * 11)                # T <= h_T: no T bump
    assert _hip.jd_scenario_layout(jc.greeks_set(m, T_=1 / 400, second=False)) == (1, [0] * 7)


@pytest.mark.parametrize("model", list(jc.MODELS))
def test_groups_are_numbered_by_first_appearance(library, model):
    sc = jc.mixed_set(jc.MODELS[model])
    assert len(sc) == 16 and {s[7] for s in sc} == {False, True}
    want = jc.mixed_groups()
    assert want[0] == 7 and want[1][:7] == [0, 1, 2, 3, 4, 5, 1]
    assert _hip.jd_scenario_layout(sc) == want == jo.layout(sc)
    assert _hip.jd_scenario_layout(sc[::-1]) == jo.layout(sc[::-1])
    assert _hip.jd_scenario_layout([sc[0]]) == (1, [0])
    sixteen = [scenario(model=(False, 0.1 * (i + 1), -0.1, 0.2, 0.0)) for i in range(16)]
    assert _hip.jd_scenario_layout(sixteen) == (16, list(range(16)))


def test_the_grouping_key_is_the_doubles_themselves(library):
    layout = _hip.jd_scenario_layout
    assert 0.1 + 0.2 != 0.3
    assert layout([scenario(T_=0.3), scenario(T_=0.1 + 0.2), scenario(T_=0.3)]) == (2, [0, 1, 0])
    assert layout([scenario(model=(False, 0.3, -0.1, 0.2, 0.0)), scenario(model=(False, 0.1 + 0.2, -0.1, 0.2, 0.0))]) == (2, [0, 1])
    # spot, strike, rates, sigma and call / put never split a group
    assert layout([scenario(), scenario(90.0, 80.0, T, 0.0, 0.35, 0.1, False)]) == (1, [0, 0])
    # a Merton a3 is unread and does not split; Kou's does; every other model field does, in both families
    assert layout([scenario(model=(False, 0.5, -0.1, 0.2, 0.0)), scenario(model=(False, 0.5, -0.1, 0.2, 7.0))]) == (1, [0, 0])
    assert layout([scenario(model=(True, 0.5, 0.4, 10.0, 5.0)), scenario(model=(True, 0.5, 0.4, 10.0, 7.0))]) == (2, [0, 1])
    for base in (jc.MERTON, jc.KOU):
        for at in (1, 2, 3):
            bumped = list(base)
            bumped[at] = base[at] * 1.5
            assert layout([scenario(model=base), scenario(model=tuple(bumped))]) == (2, [0, 1]), (base, at)
        assert layout([scenario(model=base), scenario(T_=0.5, model=base)]) == (2, [0, 1])
    assert layout([scenario(model=(False, 0.5, 0.4, 10.0, 5.0)), scenario(model=(True, 0.5, 0.4, 10.0, 5.0))]) == (2, [0, 1])


def test_layout_refuses_what_it_cannot_number(library):
    arr, _k = _hip._jd_scenarios([scenario()] * 16)
    n_groups, group = C.c_int32(-1), (C.c_int32 * 17)()
    for bad_k in (0, 17, -1):
        refused(library, library.oljs_layout(arr, bad_k, C.byref(n_groups), group), "the number of scenarios must be in [1, OLMC_MAX_BATCH]")
    refused(library, library.oljs_layout(None, 1, C.byref(n_groups), group), "null pointer")
    refused(library, library.oljs_layout(arr, 1, None, group), "null pointer")
    refused(library, library.oljs_layout(arr, 1, C.byref(n_groups), None), "null pointer")


# -------------------------------------------------------------------------------------------------------- the fold ----
def test_the_oracles_philox_is_the_c_oracles():
    paths = [0, 1, 77, (1 << 32) - 1, (1 << 32) + 5, (1 << 40) + 3]
    for block, tag, seed in ((0, 2, 1), (7, 3, 0x0123456789ABCDEF), (31, 5, (1 << 64) - 1)):
        words = jo.philox(paths, block, tag, seed)
        for i, p in enumerate(paths):
            assert list(words[:, i]) == jo.po.philox((p & 0xFFFFFFFF, p >> 32, block, tag), (seed & 0xFFFFFFFF, seed >> 32))


@pytest.mark.parametrize("n", jc.TIE_STEPS)
def test_the_folded_sums_are_the_interleaved_sums_to_rounding(n):
    """Z, J and x as the header defines them against the step-by-step running sum of oracle/philox_gbm.c, for every scenario of every set
    and every (N, n, seed) of the device's tie test, at that test's bar."""
    worst = 0.0
    for N in jc.TIE_PATHS:
        seed = jc.tie_seed(n, N)
        for label, scenarios in jc.tie_sets(n).items():
            folded = jo.payoffs(scenarios, N, n, seed)
            for i, (sc, x) in enumerate(zip(scenarios, folded)):
                paths = jo.po.jump_paths(sc[0], sc[2], sc[3], sc[4], sc[5], *sc[7:], N, n, seed)
                y = jo.payoff(paths[n], sc)
                for got, want in ((np.sum(x), np.sum(y)), (np.sum(x * x), np.sum(y * y))):
                    assert float(got) == pytest.approx(float(want), **TIE), (label, n, N, i)
                    if want > 0:
                        worst = max(worst, abs(float(got) - float(want)) / float(want))
    print(f"n = {n}: worst relative difference of a sum {worst:.3e}")


# ---------------------------------------------------------------------------------------------- the C ABI's refusals ----
def _sc(*scenarios):
    return _hip._jd_scenarios(list(scenarios) or [scenario()])


def _model(m=jc.MERTON):
    return C.byref(_hip.jd_model(*m))


_G = (S, K, T, R, SIGMA, Q, 1)
_TOO_MANY = "lambda_j * T / n_steps must be <= 20 jumps per step: raise n_steps"
_REFUSALS = [
    ("oljs_scenarios", lambda: (None, 1, 0, 100, 4, 1, 0, _out17()), "null pointer"),
    ("oljs_scenarios", lambda: (*_sc(), 0, 100, 4, 1, 0, None), "null pointer"),
    ("oljs_scenarios", lambda: (_sc()[0], 0, 0, 100, 4, 1, 0, _out17()), "the number of scenarios must be in [1, OLMC_MAX_BATCH]"),
    ("oljs_scenarios", lambda: (_sc()[0], 17, 0, 100, 4, 1, 0, _out17()), "the number of scenarios must be in [1, OLMC_MAX_BATCH]"),
    ("oljs_scenarios", lambda: (*_sc(scenario(), scenario(T_=0.0)), 0, 100, 4, 1, 0, _out17()), "T must be > 0 in every scenario"),
    ("oljs_scenarios", lambda: (*_sc(scenario(T_=-1.0)), 0, 100, 4, 1, 0, _out17()), "T must be > 0 in every scenario"),
    ("oljs_scenarios", lambda: (_hip.JsScenario(S, K, T, R, SIGMA, Q, 1, 2, 0.5, -0.1, 0.2, 0.0), 1, 0, 100, 4, 1, 0, _out17()), "bad jump model"),
    ("oljs_scenarios", lambda: (_hip.JsScenario(S, K, T, R, SIGMA, Q, 1, -1, 0.5, -0.1, 0.2, 0.0), 1, 0, 100, 4, 1, 0, _out17()), "bad jump model"),
    ("oljs_scenarios", lambda: (*_sc(scenario(), scenario(model=(False, -0.5, -0.1, 0.2, 0.0))), 0, 100, 4, 1, 0, _out17()), "lambda_j must be non-negative"),
    ("oljs_scenarios", lambda: (*_sc(scenario(), scenario(model=jc.KOU)), 0, 100, 2, 1, 0, _out17()), _TOO_MANY),
    ("oljs_scenarios", lambda: (*_sc(scenario(T_=2.0, model=jc.KOU)), 0, 100, 5, 1, 0, _out17()), _TOO_MANY),
    ("oljs_scenarios", lambda: (*_sc(), 0, 0, 4, 1, 0, _out17()), "n_paths must be >= 1"),
    ("oljs_scenarios", lambda: (*_sc(), 0, 100, 0, 1, 0, _out17()), "n_steps must be >= 1"),
    ("oljs_scenarios", lambda: (*_sc(), -1, 100, 4, 1, 0, _out17()), "path_offset must be >= 0"),
    ("oljs_greeks_fd", lambda: (*_G, _model(), 100, 4, 1, 0, 1, None, None), "null pointer"),
    ("oljs_greeks_fd", lambda: (*_G, None, 100, 4, 1, 0, 1, _out9(), None), "null pointer"),
    ("oljs_greeks_fd", lambda: (S, K, 0.0, R, SIGMA, Q, 1, _model(), 100, 4, 1, 0, 1, _out9(), None), "T must be > 0"),
    ("oljs_greeks_fd", lambda: (S, K, float("nan"), R, SIGMA, Q, 1, _model(), 100, 4, 1, 0, 1, _out9(), None), "T must be > 0"),
    ("oljs_greeks_fd", lambda: (*_G, C.byref(_hip.JdModel(2, 0, 0.5, -0.1, 0.2, 0.0)), 100, 4, 1, 0, 1, _out9(), None), "bad jump model"),
    ("oljs_greeks_fd", lambda: (*_G, _model((False, -0.5, -0.1, 0.2, 0.0)), 100, 4, 1, 0, 1, _out9(), None), "lambda_j must be non-negative"),
    ("oljs_greeks_fd", lambda: (*_G, _model(jc.KOU), 100, 2, 1, 0, 1, _out9(), None), _TOO_MANY),
    ("oljs_greeks_fd", lambda: (*_G, _model(), 0, 4, 1, 0, 1, _out9(), None), "n_paths must be >= 1"),
    ("oljs_greeks_fd", lambda: (*_G, _model(), 100, 0, 1, 0, 1, _out9(), None), "n_steps must be >= 1"),
    # two faults at once: the list before the scenarios, the scenarios before the counts, T before the model
    ("oljs_scenarios", lambda: (_sc(scenario(T_=0.0))[0], 17, 0, 0, 4, 1, 0, _out17()), "the number of scenarios must be in [1, OLMC_MAX_BATCH]"),
    ("oljs_scenarios", lambda: (*_sc(scenario(model=(False, -0.5, -0.1, 0.2, 0.0))), 0, 0, 4, 1, 0, _out17()), "lambda_j must be non-negative"),
    ("oljs_scenarios", lambda: (*_sc(scenario(T_=0.0, model=(False, -0.5, -0.1, 0.2, 0.0))), -1, 100, 4, 1, 0, _out17()), "T must be > 0 in every scenario"),
    ("oljs_scenarios", lambda: (*_sc(scenario(T_=0.0)), 0, 100, 0, 1, 0, _out17()), "n_steps must be >= 1"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    """Each refusal answers OLMC_ERR_ARG (1) with its exact message, ahead of any device work (no device is initialised here)."""
    refused(library, getattr(library, name)(*args()), message)


# ---------------------------------------------------------------------------------------------- the Python refusals ----
GOOD = dict(S=S, K=K, T=T, r=R, sigma=SIGMA)


@pytest.mark.parametrize("model", list(jc.MODELS))
@pytest.mark.parametrize("scenarios,kw,match", [
    ([], dict(), "empty"),
    ([dict(S=S, K=K, r=R, sigma=SIGMA)], dict(), "lacks"),
    ([GOOD, dict(S=S, K=K, T=T, r=R)], dict(), "scenario 1 lacks"),
    ([dict(GOOD, T=0.0)], dict(), "T must be > 0"),
    ([dict(GOOD, T=-1.0)], dict(), "T must be > 0"),
    ([dict(GOOD, vol=0.2)], dict(), "unknown"),
    ([dict(GOOD, kappa=2.0)], dict(), "unknown"),
    ([GOOD], dict(n_paths=0), ">= 1"),
    ([GOOD], dict(n_steps=0), ">= 1"),
])
def test_price_scenarios_refuses_before_the_device(no_library, model, scenarios, kw, match):
    m = ol.KouJumpDiffusion(*jc.KOU[1:]) if model == "kou" else ol.MertonJumpDiffusion(*jc.MERTON[1:4])
    with pytest.raises(ValueError, match=match):
        m.price_scenarios(scenarios, **{"n_paths": 100, "n_steps": 8, "seed": 1, **kw})


def test_a_scenarios_model_fields_are_validated_as_the_constructors_validate_them(no_library):
    merton, kou = ol.MertonJumpDiffusion(0.5, -0.1, 0.2), ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0)
    for model, fields, match in ((merton, dict(lambda_j=-1.0), "scenario 0: lambda_j must be non-negative"), (merton, dict(sigma_j=-0.1), "sigma_j must be non-negative"),
                                 (kou, dict(p=1.5), "p must be in"), (kou, dict(eta1=1.0), "eta1 must be > 1"), (kou, dict(eta2=0.0), "eta2 must be positive"),
                                 (merton, dict(eta1=12.0), "unknown"), (kou, dict(mu_j=0.1), "unknown")):
        with pytest.raises(ValueError, match=match):
            model.price_scenarios([dict(GOOD, **fields)], 100, 8, 1)
    assert (merton.lambda_j, merton.mu_j, merton.sigma_j) == (0.5, -0.1, 0.2)


@pytest.mark.parametrize("kw", [dict(n_paths=0), dict(n_steps=0)])
def test_the_adapter_refuses_before_the_device(no_library, kw):
    for m in (ol.MertonJumpDiffusion(0.5, -0.1, 0.2), ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0)):
        with pytest.raises(ValueError, match=">= 1"):
            ol.JumpMCAdapter(m, **{"n_paths": 100, "n_steps": 8, "seed": 1, **kw})
        with pytest.raises(ValueError, match=">= 1"):
            ol.greeks_jump_monte_carlo(m, S, K, T, R, SIGMA, **{"n_paths": 100, "n_steps": 8, "seed": 1, **kw})


def test_the_adapter_reaches_the_device_only_to_price(no_library):
    m = ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0)
    adapter = ol.JumpMCAdapter(m, 100, 8)
    assert isinstance(adapter.seed, int) and adapter._can_fuse({}) and not adapter._can_fuse({"seed": 1})
    assert ol.JumpMCAdapter(m, 100, 8, seed=5, antithetic=True).seed == 5
    with pytest.raises(AssertionError, match="loaded"):
        adapter.price(S, K, T, R, 0.25, "call", Q)
    with pytest.raises(ol.GreeksError, match="loaded"):
        ol.compute_greeks_unified(adapter, S, K, T, R, SIGMA, "call", Q)


def test_the_new_names_are_exported():
    for name in ("JumpMCAdapter", "greeks_jump_monte_carlo"):
        assert name in ol.__all__ and hasattr(ol, name)
    for cls in (ol.MertonJumpDiffusion, ol.KouJumpDiffusion):
        assert hasattr(cls, "price_scenarios")


def test_price_scenarios_cuts_forty_scenarios_in_the_callers_order_with_one_seed(monkeypatch):
    calls = []

    def fake(scenarios, n_paths, n_steps, seed, antithetic=False, path_offset=0):
        calls.append((list(scenarios), n_paths, n_steps, seed, antithetic))
        out = []
        for sc in scenarios:
            st = _hip.Stats()
            st.price, st.std_error = sc[1], sc[8]                                    # the strike and lambda_j come back: the order is checked below
            out.append(st)
        return out

    monkeypatch.setattr(_hip, "jd_scenarios", fake)
    m = ol.MertonJumpDiffusion(0.5, -0.1, 0.2)
    scenarios = [dict(GOOD, K=50.0 + i, lambda_j=0.1 * (i % 7)) for i in range(40)]
    scenarios[3].update(q=0.03, option_type="put", sigma_j=0.3)
    prices, errors = m.price_scenarios(scenarios, 100, 8, None, True, return_error=True)
    assert [len(c[0]) for c in calls] == [16, 16, 8]
    assert calls[0][3] == calls[1][3] == calls[2][3] and all(c[1:3] == (100, 8) and c[4] is True for c in calls)
    assert list(prices) == [50.0 + i for i in range(40)] and list(errors) == [0.1 * (i % 7) for i in range(40)]
    assert prices.dtype == np.float64 and prices.shape == (40,)
    assert calls[0][0][0] == (S, 50.0, T, R, SIGMA, 0.0, True, False, 0.0, -0.1, 0.2, 0.0)
    assert calls[0][0][3] == (S, 53.0, T, R, SIGMA, 0.03, False, False, 0.1 * 3, -0.1, 0.3, 0.0)
    kou = ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0)
    only = kou.price_scenarios([dict(GOOD, eta2=6.0)], 100, 8, 3)
    assert only.shape == (1,) and calls[-1][3] == 3 and calls[-1][0][0][7:] == (True, 1.0, 0.4, 10.0, 6.0)


# ------------------------------------------------------------------------------------------ the fold under sanitizers ----
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("jump_scenarios") / "jump_scenario_san"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "optionslab_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "jump_scenario_harness.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed: " + build.stderr.splitlines()[0])
    assert build.returncode == 0, build.stderr

    def run(*args, stdin=""):
        r = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True,
                           env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
        assert r.returncode == 0, r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    return run


def test_property_sweep_is_clean_under_asan_and_ubsan(harness):
    """4,000 random scenario lists (1 .. 16 scenarios from pools of 1 .. 16 jump laws of both families, NaN strikes among them): the
    grouping against a brute-force one, the kernel's slots a permutation sorted by group that carries each scenario's own constants by
    the one-contract kernels' products, a group's first slot forming its own spot; the Greeks' scenarios for 7 / 8 / 11 / 14 contracts."""
    out = harness("self")
    assert out.startswith("ok ") and int(out.split()[1]) > 100_000


def test_grouping_in_the_header_is_the_grouping_the_library_reports(library, harness):
    """oljs_layout of the built libolmc.so (a pure host entry point: no device) == the header compiled by g++."""
    for model in jc.MODELS.values():
        for sc in (jc.mixed_set(model), jc.mixed_set(model)[::-1][:9], jc.greeks_set(model)):
            lines = "\n".join(" ".join(repr(float(x)) for x in s[:6]) + f" {int(s[6])} {int(s[7])} " + " ".join(repr(float(x)) for x in s[8:]) for s in sc)
            out = harness("layout", len(sc), stdin=lines).split()
            n_groups, group = _hip.jd_scenario_layout(sc)
            assert [int(x) for x in out] == [n_groups, *group]
