"""CPU checks of the path-dependent jump-diffusion entry points (include/olmc_jump.h, MertonJumpDiffusion / KouJumpDiffusion).

  ABI      olmc_jump.h's declarations = the library's oljd_* exports = _hip.JD_PROTOTYPES; the header is plain C; oljd_model's layout is
           the ctypes structure's; olmc.h's catalogue and the ABI version stay as they are.
  Python   the six new methods keep HestonPricer's parameter names and defaults (no method= / scheme=), raise their ValueErrors before the
           library is loaded, and compat.install() still exposes both classes.
"""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys

import optionslab_amd as ol
from optionslab_amd import _hip
from tests.abi_support import assert_header_matches, library, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc_jump.h")
NAMES = ["oljd_autocallable", "oljd_cliquet", "oljd_paths", "oljd_price", "oljd_surface_prices"]
METHODS = ("price_asian", "price_barrier", "price_lookback", "price_surface", "price_autocallable", "price_cliquet")


def c_compiler():
    from optionslab_amd.build import _hipcc

    cc = shutil.which("cc") or shutil.which("gcc")
    return [cc] if cc else [_hipcc(), "-x", "c"]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_header.c"
    src.write_text('#include "olmc_jump.h"\n'
                   "int use(const oljd_model* m, olmc_stats* out) {\n"
                   "    return oljd_price(100, 100, 1, 0.05, 0.2, 0, 1, m, OLJD_EUROPEAN, 0, 0, 1000, 8, 1, 0, out); }\n")
    subprocess.run([*c_compiler(), "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(src)], check=True)


def test_header_exports_and_prototypes_agree(library):
    assert_header_matches(library, HEADER, "oljd_", _hip.JD_PROTOTYPES, NAMES)
    assert _hip.JD_EUROPEAN == 8 == _hip.LV_EUROPEAN


def test_the_model_struct_has_the_headers_layout(tmp_path):
    fields = ("model", "pad", "lambda_j", "a1", "a2", "a3")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "olmc_jump.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu", sizeof(oljd_model));\n'
                   + "".join(f'    printf(" %zu", offsetof(oljd_model, {f}));\n' for f in fields)
                   + '    printf(" %d %d %d", OLJD_EUROPEAN, OLMC_JUMP_MERTON, OLMC_JUMP_KOU);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([*c_compiler(), "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_hip.JdModel)] + [getattr(_hip.JdModel, f).offset for f in fields] + [_hip.JD_EUROPEAN, 0, 1]
    assert got[:7] == [40, 0, 4, 8, 16, 24, 32]
    m = _hip.jd_model(True, 1.5, 0.4, 10.0, 5.0)
    assert (m.model, m.pad, m.lambda_j, m.a1, m.a2, m.a3) == (1, 0, 1.5, 0.4, 10.0, 5.0)
    assert _hip.jd_model(False, 0.5, -0.1, 0.2).a3 == 0.0


def test_every_refusal_answers_its_message_before_any_device_work(library):
    """rc 1 (OLMC_ERR_ARG) and the exact words, on a machine with or without a device: none of these calls initialises one."""
    S, K, T, R, SIGMA, Q, N, n = 100.0, 100.0, 1.0, 0.05, 0.2, 0.01, 100, 12
    good = _hip.jd_model(False, 0.5, -0.1, 0.2)
    out, cells = _hip.Stats(), (_hip.Stats * 16)()
    strikes, steps = (C.c_double * 16)(*([K] * 16)), (C.c_int32 * 16)(*([n] * 16))
    buf = (C.c_double * 8)()

    def entries(m, n_steps=n, offset=0, count=N, payoff=6, barrier=0.0, k=1, freq=3, periods=4, st=True):
        o = C.byref(out) if st else None
        return {"oljd_price": lambda: library.oljd_price(S, K, T, R, SIGMA, Q, 1, m, payoff, barrier, offset, count, n_steps, 1, 0, o),
                "oljd_surface_prices": lambda: library.oljd_surface_prices(S, T, R, SIGMA, Q, 1, m, strikes, steps, k, offset, count, n_steps, 1, 0,
                                                                           cells if st else None),
                "oljd_autocallable": lambda: library.oljd_autocallable(S, T, R, SIGMA, Q, m, 1.0, 0.9, 0.1, 0.8, freq, offset, count, n_steps, 1, 0, o),
                "oljd_cliquet": lambda: library.oljd_cliquet(S, T, R, SIGMA, Q, m, 0.05, -0.05, 0.3, 0.0, periods, offset, count, n_steps, 1, 0, o),
                "oljd_paths": lambda: library.oljd_paths(S, T, R, SIGMA, Q, m, count, n_steps, 1, 0, 1, buf if st else None)}

    def every(message, skip=(), **kw):
        for name, call in entries(**kw).items():
            if name not in skip:
                refused(library, call(), message)

    every("null pointer", m=None)
    every("null pointer", m=C.byref(good), st=False)
    refused(library, library.oljd_surface_prices(S, T, R, SIGMA, Q, 1, C.byref(good), None, steps, 1, 0, N, n, 1, 0, cells), "null pointer")
    refused(library, library.oljd_surface_prices(S, T, R, SIGMA, Q, 1, C.byref(good), strikes, None, 1, 0, N, n, 1, 0, cells), "null pointer")
    for code in (2, -1):
        every("bad jump model", m=C.byref(_hip.JdModel(code, 0, 0.5, -0.1, 0.2, 0.0)))
    every("lambda_j must be non-negative", m=C.byref(_hip.jd_model(False, -0.5, -0.1, 0.2)))
    every("lambda_j * T / n_steps must be <= 20 jumps per step: raise n_steps", m=C.byref(_hip.jd_model(True, 60.0, 0.6, 25.0, 20.0)), n_steps=2)
    every("n_steps must be >= 1", m=C.byref(good), n_steps=0)
    every("n_paths must be >= 1", m=C.byref(good), count=0)
    every("path_offset must be >= 0", m=C.byref(good), offset=-1, skip=("oljd_paths",))
    for payoff in (-1, 9):
        refused(library, entries(C.byref(good), payoff=payoff)["oljd_price"](), "bad payoff")
    for kind in range(4):
        for level in (0.0, -5.0):
            refused(library, entries(C.byref(good), payoff=kind, barrier=level)["oljd_price"](), "Barrier must be positive")
    for k in (0, 17):
        refused(library, entries(C.byref(good), k=k)["oljd_surface_prices"](), "the number of cells must be in [1, OLMC_MAX_BATCH]")
    for bad_step in (0, n + 1):
        two = (C.c_int32 * 2)(n, bad_step)
        refused(library, library.oljd_surface_prices(S, T, R, SIGMA, Q, 1, C.byref(good), strikes, two, 2, 0, N, n, 1, 0, cells),
                "a cell's step must be in [1, n_steps]")
    refused(library, entries(C.byref(good), freq=0)["oljd_autocallable"](), "observation_freq must be >= 1")
    refused(library, entries(C.byref(good), freq=n + 1)["oljd_autocallable"](), "no observation date: observation_freq > n_steps")
    for periods in (0, n + 1):
        refused(library, entries(C.byref(good), periods=periods)["oljd_cliquet"](), "n_periods must be in [1, n_steps]")
    refused(library, entries(C.byref(good), count=1 << 27, n_steps=252)["oljd_paths"](), "path matrix would exceed 64 GB")
    # two faults at once: the model comes first
    refused(library, entries(C.byref(_hip.JdModel(2, 0, 0.5, -0.1, 0.2, 0.0)), payoff=9)["oljd_price"](), "bad jump model")
    refused(library, entries(C.byref(good), payoff=9, count=0)["oljd_price"](), "bad payoff")
    # the model's checks hold the step count (make_jump), so it comes before the payoff; the path count before the cells
    refused(library, entries(C.byref(good), payoff=9, n_steps=0)["oljd_price"](), "n_steps must be >= 1")
    two = (C.c_int32 * 2)(n, n + 1)
    refused(library, library.oljd_surface_prices(S, T, R, SIGMA, Q, 1, C.byref(good), strikes, two, 2, 0, 0, n, 1, 0, cells), "n_paths must be >= 1")
    refused(library, entries(C.byref(good), k=17, count=0)["oljd_surface_prices"](), "n_paths must be >= 1")
    refused(library, entries(C.byref(good), n_steps=0, count=0)["oljd_paths"](), "n_steps must be >= 1")
    refused(library, entries(C.byref(good), count=0, n_steps=1 << 30)["oljd_paths"](), "n_paths must be >= 1")


def models():
    return ol.MertonJumpDiffusion(0.5, -0.1, 0.2), ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0)


def test_the_new_methods_keep_the_heston_pricers_names_and_defaults():
    for model in models():
        for name in METHODS:
            mine = inspect.signature(getattr(type(model), name)).parameters
            theirs = inspect.signature(getattr(ol.HestonPricer, name)).parameters
            assert "sigma" in mine and mine["sigma"].default is inspect.Parameter.empty, name
            assert not {"method", "scheme", "path_construction"} & set(mine), name
            assert set(mine) - {"sigma"} == set(theirs) - {"method", "scheme", "path_construction"}, name
            for p in set(mine) & set(theirs):
                assert mine[p].default == theirs[p].default and mine[p].kind == theirs[p].kind, (name, p)
            order = list(mine)
            assert order.index("sigma") == order.index("r") + 1, name                  # where price_monte_carlo has it
            assert [p for p in order if p != "sigma"] == [p for p in theirs if p in mine], name
        for name, extra in (("price_monte_carlo", "antithetic"), ("simulate_paths", "mirror")):
            p = inspect.signature(getattr(type(model), name)).parameters[extra]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, name
        assert list(inspect.signature(type(model).price_monte_carlo).parameters)[:6] == ["self", "S", "K", "T", "r", "sigma"]


def test_value_errors_come_before_the_library_is_loaded():
    code = (
        "import pytest, optionslab_amd as ol\n"
        "from optionslab_amd import _hip\n"
        "for m in (ol.MertonJumpDiffusion(0.5, -0.1, 0.2), ol.KouJumpDiffusion(1.0, 0.4, 10.0, 5.0)):\n"
        "    bad = [lambda **kw: m.price_asian(100, 100, 1.0, 0.05, 0.2, **kw), lambda **kw: m.price_barrier(100, 100, 1.0, 0.05, 0.2, 120.0, **kw),\n"
        "           lambda **kw: m.price_lookback(100, 100, 1.0, 0.05, 0.2, **kw), lambda **kw: m.price_surface(100, [100.0], [1.0], 0.05, 0.2, **kw),\n"
        "           lambda **kw: m.price_autocallable(100, 1.0, 0.05, 0.2, **kw), lambda **kw: m.price_cliquet(100, 1.0, 0.05, 0.2, **kw),\n"
        "           lambda **kw: m.price_monte_carlo(100, 100, 1.0, 0.05, 0.2, antithetic=True, **kw),\n"
        "           lambda **kw: m.simulate_paths(100, 1.0, 0.05, 0.2, mirror=True, **kw)]\n"
        "    for call in bad:\n"
        "        for kw in (dict(n_paths=0), dict(n_steps=0)):\n"
        "            with pytest.raises(ValueError, match='n_paths and n_steps must be >= 1'):\n"
        "                call(**kw)\n"
        "    with pytest.raises(ValueError, match='avg_type'):\n"
        "        m.price_asian(100, 100, 1.0, 0.05, 0.2, avg_type='harmonic')\n"
        "    with pytest.raises(ValueError, match='Barrier must be positive'):\n"
        "        m.price_barrier(100, 100, 1.0, 0.05, 0.2, 0.0)\n"
        "    with pytest.raises(ValueError, match='lookback_type'):\n"
        "        m.price_lookback(100, 100, 1.0, 0.05, 0.2, lookback_type='partial')\n"
        "    with pytest.raises(ValueError, match='observation_freq must be >= 1'):\n"
        "        m.price_autocallable(100, 1.0, 0.05, 0.2, observation_freq=0)\n"
        "    for periods in (0, 13):\n"
        "        with pytest.raises(ValueError, match='n_periods must be in'):\n"
        "            m.price_cliquet(100, 1.0, 0.05, 0.2, n_periods=periods, n_steps=12)\n"
        "    with pytest.raises(ValueError, match='strikes must not be empty'):\n"
        "        m.price_surface(100, [], [1.0], 0.05, 0.2)\n"
        "    with pytest.raises(ValueError, match='not on the grid'):\n"
        "        m.price_surface(100, [100.0], [1.0, 0.3], 0.05, 0.2, n_steps=4)\n"
        "    assert m.price_barrier.__doc__ and m.price_surface.__doc__\n"
        "assert _hip._lib is None, 'the library was loaded'\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_compat_still_exposes_both_classes():
    from optionslab_amd import compat

    was_installed = bool(compat._installed)
    compat.install()
    try:
        from src.pricing_models.jump_diffusion import KouJumpDiffusion, MertonJumpDiffusion

        assert MertonJumpDiffusion is ol.MertonJumpDiffusion and KouJumpDiffusion is ol.KouJumpDiffusion
        assert all(hasattr(cls, name) for cls in (MertonJumpDiffusion, KouJumpDiffusion) for name in METHODS)
        assert sorted(vars(sys.modules["src.pricing_models.jump_diffusion"]).keys() - {"__name__", "__doc__", "__package__", "__loader__", "__spec__"}) \
            == ["KouJumpDiffusion", "MertonJumpDiffusion", "__optionslab_amd__"]
    finally:
        if not was_installed:
            compat.uninstall()
