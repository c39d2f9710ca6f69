"""CPU checks of the C-ABI boundary: libolmc.so builds/loads, exports every
symbol include/olmc.h declares, the ctypes prototypes cover them all, struct
layouts match, the pure host function works, and -- without a GPU -- compute
entry points fail loudly instead of falling back."""
import ctypes as C
import os
import re
import subprocess

import pytest

from optionslab_amd import _hip
from optionslab_amd.build import LIBRARY
from optionslab_amd.exceptions import AccelerationError
from tests.abi_support import _CV, _ST, _opts, _out9, library, refused, sobol as _sobol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olmc.h")
PROBE_HEADER = os.path.join(ROOT, "include", "olmc_probe.h")


def declared_symbols(header=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(olmc_[a-z0-9_]+)\s*\(", text)))


def exported_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bT (olmc_[a-z0-9_]+)", out))


def test_header_declares_the_expected_surface():
    names = declared_symbols()
    for must in ("olmc_init", "olmc_european", "olmc_european_batch", "olmc_european_greeks_fd", "olmc_european_terminal",
                 "olmc_european_cv", "olmc_asian", "olmc_multi_gpu_european", "olmc_last_error", "olmc_shutdown"):
        assert must in names


def test_library_exports_every_declared_symbol(library):
    for name in declared_symbols():
        assert hasattr(library, name), f"{name} declared in include/olmc.h but not exported"
    assert set(declared_symbols()) == exported_symbols(LIBRARY)      # nothing undeclared is exported either


def test_measurement_code_is_not_in_the_product_library():
    """probe / stamp / clock / moment kernels, their entry points and the fault-injection knobs live in the
    instrumented build (include/olmc_probe.h -> tools/probe/libolmc_probe.so), which also exports the whole pricing ABI."""
    from optionslab_amd.build import PROBE_LIBRARY, build_probe_library
    from tools.probe import binding as probe

    build_probe_library()
    product, instrumented = exported_symbols(LIBRARY), exported_symbols(PROBE_LIBRARY)
    only_probe = set(declared_symbols(PROBE_HEADER))
    assert only_probe == set(probe.PROBE_PROTOTYPES) and len(only_probe) == 17
    assert not (only_probe & product)
    assert not [n for n in product if any(w in n for w in ("probe", "stamp", "clock", "moments"))]
    assert instrumented == product | only_probe
    blob = open(LIBRARY, "rb").read()
    for word in (b"probe_mad_u64_u32", b"european_stamp_kernel", b"clock_probe_kernel", b"normal_moments_kernel", b"ha_fit_probe_kernel",
                 b"lsm_fit_probe_kernel", b"rows_store_probe_kernel", b"rows_total_probe_kernel", b"FAULT_SHARD", b"injected shard failure"):
        assert word not in blob, word
    probe_blob = open(PROBE_LIBRARY, "rb").read()
    for word in (b"european_stamp_kernel", b"ha_fit_probe_kernel", b"lsm_fit_probe_kernel", b"rows_store_probe_kernel", b"rows_total_probe_kernel"):
        assert word in probe_blob, word
    lib = probe.hip.load_library()
    for name in only_probe:
        assert hasattr(lib, name)


def test_ctypes_prototypes_cover_the_header():
    assert sorted(_hip.PROTOTYPES) == declared_symbols()


def test_library_carries_gfx950_code_object():
    blob = open(LIBRARY, "rb").read()
    assert b"gfx950" in blob


def test_struct_layouts_match_the_header():
    assert C.sizeof(_hip.Stats) == 40
    assert C.sizeof(_hip.Option) == 56
    assert C.sizeof(_hip.CvMoments) == 56
    assert _hip.Stats.n.offset == 16 and _hip.Stats.price.offset == 24


def test_abi_version_and_error_string(library):
    assert library.olmc_abi_version() == 6
    assert isinstance(library.olmc_last_error(), bytes)


def test_combine_stats_is_a_pure_host_function(library):
    # two shards of payoffs {1,2,3} and {4}: mean 2.5, var(ddof=0) 1.25
    st = _hip.combine_stats([(6.0, 14.0, 3), (4.0, 16.0, 1)], r=0.0, T=1.0)
    assert st.n == 4 and st.sum == 10.0 and st.sumsq == 30.0
    assert st.price == 2.5
    assert abs(st.std_error - (1.25 ** 0.5) / 2.0) < 1e-15
    with pytest.raises(AccelerationError):
        _hip.combine_stats([], 0.0, 1.0)


def _no_gpu():
    return not os.path.exists("/dev/kfd")


@pytest.mark.skipif(not _no_gpu(), reason="GPU present: loud-failure path not reachable")
def test_compute_fails_loudly_without_a_gpu():
    with pytest.raises(AccelerationError) as e:
        _hip.european(100, 100, 1.0, 0.05, 0.2, 0.0, True, 1000, 4, 1)
    assert e.value.backend == "hip"
    import optionslab_amd as ol
    with pytest.raises(AccelerationError):
        ol.MonteCarloPricer(1000, 4, 1).price(100, 100, 1.0, 0.05, 0.2, "call")
    with pytest.raises(ol.GreeksError):
        ol.compute_greeks_unified(ol.MonteCarloPricer(1000, 4, 1), 100, 100, 1.0, 0.05, 0.2)
    with pytest.raises(AccelerationError):
        ol.AsianOption(100, 100, 1.0, 0.05, 0.2, seed=1).price(100, 8)
    with pytest.raises(AccelerationError):
        ol.simulate_gbm_hip(100, 1.0, 0.05, 0.2, 0.0, 100, 4, 1)
    assert ol.hip_available() is False and ol.HIP_AVAILABLE is False


def _build_c_example(tmp_path, name="price_from_c", extra=()):
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    _hip.load_library()                                   # builds libolmc.so if it is stale
    exe = str(tmp_path / name)
    pkg = os.path.join(root, "optionslab_amd")
    subprocess.run([cc, "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", *extra, "-I" + os.path.join(root, "include"),
                    os.path.join(root, "examples", name + ".c"), "-o", exe, "-L" + pkg, "-lolmc", "-Wl,-rpath," + pkg], check=True)
    return exe


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present: the example runs in the gpu suite")
def test_header_is_plain_c_and_a_c_host_fails_loudly_without_a_gpu(tmp_path):
    """include/olmc.h compiles as C99 with -Werror and links against libolmc.so; with no device the host gets a
    status code and a message, not a crash and not a CPU answer."""
    import subprocess

    out = subprocess.run([_build_c_example(tmp_path), "1000", "10"], capture_output=True, text=True)
    assert out.returncode == 1 and "olmc_init(0) failed" in out.stderr and "european" not in out.stdout


@pytest.mark.gpu
def test_c_host_example_prices_on_the_gpu(tmp_path):
    import re
    import subprocess

    out = subprocess.run([_build_c_example(tmp_path), "200000", "50"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    price = float(re.search(r"european call\s+price ([0-9.]+)", out.stdout).group(1))
    assert abs(price - 10.450583572185565) < 0.2 and "two shards" in out.stdout and "asian call" in out.stdout


def test_the_threaded_c_host_compiles_against_the_header(tmp_path):
    _build_c_example(tmp_path, "threads_from_c", extra=("-pthread",))


@pytest.mark.gpu
def test_c_host_threads_price_concurrently_with_identical_bits(tmp_path):
    import json
    import subprocess

    out = subprocess.run([_build_c_example(tmp_path, "threads_from_c", extra=("-pthread",)), "10000", "50", "0.3"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [r["threads"] for r in rows] == [1, 2, 4, 8, 16] and all(r["bit_identical_results"] for r in rows)
    assert max(r["calls_per_s"] for r in rows[1:]) > rows[0]["calls_per_s"]          # concurrent callers are not serialised


def test_the_kernels_refuse_a_finite_math_build():
    """dead lanes are zeroed by fmax(NaN, 0) = 0; -ffinite-math-only / -ffast-math would silently break that."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-ffast-math", "--cuda-device-only", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "optionslab_amd", "csrc"), os.path.join(ROOT, "optionslab_amd", "csrc", "olmc.hip")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "do not build with -ffinite-math-only" in r.stderr


# One row per argument refusal of the pricing entry points that happens before a device is touched: (entry point, arguments,
# exact olmc_last_error() message).  Every row returns OLMC_ERR_ARG with or without a GPU.
_G = (100.0, 100.0, 1.0, 0.05, 0.2, 0.0, 1)                       # S K T r sigma q is_call
_GT0 = (100.0, 100.0, 0.0, 0.05, 0.2, 0.0, 1)                     # T = 0
_MKT = (100.0, 1.0, 0.05, 0.2, 0.0)                               # S T r sigma q
_HES = (0.05, 0.0, 2.0, 0.04, 0.3)                                # r q kappa theta sigma_v (rho, v0 follow)


_REFUSALS = [
    ("olmc_european", lambda: (*_G, 0, 4, 1, 1, _ST()), "n_paths must be >= 1"),
    ("olmc_european", lambda: (*_G, 100, 0, 1, 1, _ST()), "n_steps must be >= 1"),
    ("olmc_european", lambda: (*_G, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_european_shard", lambda: (*_G, -1, 100, 4, 1, 1, _ST()), "path_offset must be >= 0"),
    ("olmc_european_shard_dev", lambda: (*_G, 0, 100, 4, 1, 1, None, None), "null pointer"),
    ("olmc_european_shard_dev", lambda: (*_G, 0, 0, 4, 1, 1, C.c_void_p(8), None), "n_paths must be >= 1"),
    ("olmc_european_batch", lambda: (_opts(2), 0, 0, 100, 4, 1, 1, (_hip.Stats * 16)()), "batch size must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_european_batch", lambda: (_opts(2), 17, 0, 100, 4, 1, 1, (_hip.Stats * 16)()), "batch size must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_european_batch", lambda: (None, 2, 0, 100, 4, 1, 1, (_hip.Stats * 16)()), "null pointer"),
    ("olmc_european_batch", lambda: (_opts(2), 2, 0, 100, 0, 1, 1, (_hip.Stats * 16)()), "n_steps must be >= 1"),
    ("olmc_european_multi", lambda: (_opts(2), None, 0, 100, 4, 1, 1, (_hip.Stats * 16)()), "n_options must be >= 1"),
    ("olmc_european_multi", lambda: (_opts(2), None, 2, 0, 4, 1, 1, (_hip.Stats * 16)()), "n_paths must be >= 1"),
    ("olmc_european_greeks_fd", lambda: (*_GT0, 100, 4, 1, 0, _out9(), None), "T must be > 0 (price() returns intrinsic value without simulating)"),
    ("olmc_european_greeks_fd", lambda: (*_G, 0, 4, 1, 0, _out9(), None), "n_paths must be >= 1"),
    ("olmc_european_terminal", lambda: (*_MKT, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_european_terminal", lambda: (*_MKT, 100, 0, 1, 1, (C.c_double * 4)()), "n_steps must be >= 1"),
    ("olmc_european_cv", lambda: (*_G, 0, 4, 1, 1, _CV()), "n_paths must be >= 1"),
    ("olmc_european_cv_shard", lambda: (*_G, -5, 100, 4, 1, 1, _CV()), "path_offset must be >= 0"),
    ("olmc_european_cv_shard", lambda: (*_G, 0, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_asian", lambda: (*_G, 7, 0, 100, 4, 1, 1, _ST()), "bad avg_kind"),
    ("olmc_asian", lambda: (*_G, 0, 0, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_asian", lambda: (*_G, 2, 0, 100, 0, 1, 1, _ST()), "n_steps must be >= 1"),
    ("olmc_asian_greeks_fd", lambda: (*_GT0, 0, 100, 4, 1, 1, 0, _out9(), None), "T must be > 0"),
    ("olmc_asian_greeks_fd", lambda: (*_G, 2, 100, 4, 1, 1, 0, _out9(), None),
     "avg_kind must be OLMC_AVG_ARITHMETIC or OLMC_AVG_GEOMETRIC (the fp32-exponent form has no fused Greeks)"),
    ("olmc_asian_greeks_fd", lambda: (*_G, 0, 0, 4, 1, 1, 0, _out9(), None), "n_paths must be >= 1"),
    ("olmc_asian_greeks_fd", lambda: (*_G, 0, 100, 4, 1, 1, 0, None, None), "null pointer"),
    ("olmc_barrier", lambda: (*_G, -1.0, 0, 0, 100, 4, 1, 1, _ST()), "Barrier must be positive"),
    ("olmc_barrier", lambda: (*_G, 120.0, 4, 0, 100, 4, 1, 1, _ST()), "bad barrier_kind"),
    ("olmc_barrier", lambda: (*_G, 120.0, 0, 0, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_barrier", lambda: (*_G, 120.0, 0, 0, 100, 0, 1, 1, _ST()), "n_steps must be >= 1"),
    ("olmc_lookback", lambda: (*_G, 1, -1, 100, 4, 1, 1, _ST()), "path_offset must be >= 0"),
    ("olmc_lookback", lambda: (*_G, 1, 0, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_extrema_greeks_fd", lambda: (*_GT0, 0, 120.0, 100, 4, 1, 1, 0, _out9(), None), "T must be > 0"),
    ("olmc_extrema_greeks_fd", lambda: (*_G, 6, 120.0, 100, 4, 1, 1, 0, _out9(), None),
     "payoff must be a barrier kind (0..3) or OLMC_LOOKBACK_FLOATING / _FIXED (4, 5)"),
    ("olmc_extrema_greeks_fd", lambda: (*_G, 2, 0.0, 100, 4, 1, 1, 0, _out9(), None), "Barrier must be positive"),
    ("olmc_extrema_greeks_fd", lambda: (*_G, 4, 0.0, 0, 4, 1, 1, 0, _out9(), None), "n_paths must be >= 1"),
    ("olmc_extrema_greeks_fd", lambda: (*_G, 4, 0.0, (1 << 26) + 1, 4, 1, 1, 0, _out9(), None),
     "n_paths beyond one launch of the fused Greeks kernel (2^26)"),
    ("olmc_autocallable", lambda: (*_MKT, 1.0, 0.8, 0.05, 0.6, 0, 0, 100, 4, 1, 1, _ST()), "observation_freq must be >= 1"),
    ("olmc_autocallable", lambda: (*_MKT, 1.0, 0.8, 0.05, 0.6, 5, 0, 100, 4, 1, 1, _ST()), "no observation date: observation_freq > n_steps"),
    ("olmc_autocallable", lambda: (*_MKT, 1.0, 0.8, 0.05, 0.6, 1, 0, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_autocallable", lambda: (*_MKT, 1.0, 0.8, 0.05, 0.6, 1, 0, 0, 4, 1, 1, _ST()), "n_paths must be >= 1"),
    ("olmc_cliquet", lambda: (*_MKT, 0.05, 0.0, 0.5, 0.0, 0, 0, 100, 4, 1, 1, _ST()), "n_periods must be in [1, n_steps]"),
    ("olmc_cliquet", lambda: (*_MKT, 0.05, 0.0, 0.5, 0.0, 5, 0, 100, 4, 1, 1, _ST()), "n_periods must be in [1, n_steps]"),
    ("olmc_cliquet", lambda: (*_MKT, 0.05, 0.0, 0.5, 0.0, 2, -1, 100, 4, 1, 1, _ST()), "path_offset must be >= 0"),
    ("olmc_gbm_paths", lambda: (*_MKT, 100, 4, 1, 0, None), "null pointer"),
    ("olmc_gbm_paths", lambda: (*_MKT, 10 ** 9, 10, 1, 0, (C.c_double * 4)()), "path matrix would exceed 64 GB"),
    ("olmc_gbm_paths", lambda: (*_MKT, 0, 10, 1, 0, (C.c_double * 4)()), "n_paths must be >= 1"),
    ("olmc_exercise_boundary", lambda: (*_G, 100, 4, 1, None), "null pointer"),
    ("olmc_exercise_boundary", lambda: (*_G, 10 ** 9, 10, 1, (C.c_double * 4)()), "path matrix would exceed 64 GB"),
    ("olmc_heston_paths", lambda: (100.0, 1.0, *_HES, 1.5, 0.04, 100, 4, 1, 0, (C.c_double * 4)(), (C.c_double * 4)()), "rho must be in [-1, 1]"),
    ("olmc_heston_paths", lambda: (100.0, 1.0, *_HES, -0.5, 0.04, 100, 4, 1, 0, (C.c_double * 4)(), None), "null pointer"),
    ("olmc_heston_paths", lambda: (100.0, 1.0, *_HES, -0.5, 0.04, 5 * 10 ** 8, 10, 1, 0, (C.c_double * 4)(), (C.c_double * 4)()),
     "path matrices would exceed 64 GB"),
    ("olmc_heston", lambda: (100.0, 100.0, 1.0, 0.05, 0.0, 1, 2.0, 0.04, 0.3, -1.5, 0.04, 0, 100, 4, 1, 1, _ST()), "rho must be in [-1, 1]"),
    ("olmc_heston", lambda: (100.0, 100.0, 1.0, 0.05, 0.0, 1, 2.0, 0.04, 0.3, -0.5, 0.04, 0, 100, 4, 1, 1, None), "null pointer"),
    ("olmc_heston", lambda: (100.0, 100.0, 1.0, 0.05, 0.0, 1, 2.0, 0.04, 0.3, -0.5, 0.04, 0, 100, 0, 1, 1, _ST()), "n_steps must be >= 1"),
    ("olmc_jump_diffusion", lambda: (*_G, 2, 1.0, -0.1, 0.2, 0.0, 0, 100, 4, 1, _ST()), "bad jump model"),
    ("olmc_jump_diffusion", lambda: (*_G, 0, -1.0, -0.1, 0.2, 0.0, 0, 100, 4, 1, _ST()), "lambda_j must be non-negative"),
    ("olmc_jump_diffusion", lambda: (*_G, 0, 100.0, -0.1, 0.2, 0.0, 0, 100, 4, 1, _ST()),
     "lambda_j * T / n_steps must be <= 20 jumps per step: raise n_steps"),
    ("olmc_jump_diffusion", lambda: (*_G, 0, 1.0, -0.1, 0.2, 0.0, 0, 100, 4, 1, None), "null pointer"),
    ("olmc_jump_paths", lambda: (*_MKT, 0, 1.0, -0.1, 0.2, 0.0, 100, 4, 1, 0, None), "null pointer"),
    ("olmc_jump_paths", lambda: (*_MKT, 0, 1.0, -0.1, 0.2, 0.0, 100, 0, 1, 0, (C.c_double * 4)()), "n_steps must be >= 1"),
    ("olmc_jump_paths", lambda: (*_MKT, 0, 1.0, -0.1, 0.2, 0.0, 10 ** 9, 10, 1, 0, (C.c_double * 4)()), "path matrix would exceed 64 GB"),
    ("olmc_american_lsm", lambda: (*_G, 100, 4, 0, 1, _ST()), "poly_degree must be in [1, 4]"),
    ("olmc_american_lsm", lambda: (*_G, 10 ** 9, 10, 2, 1, _ST()), "path matrix would exceed 64 GB: lower n_paths or n_steps"),
    ("olmc_european_qmc", lambda: (*_G, 0, 64, 4, *_sobol(4), 30, None), "null pointer"),
    ("olmc_european_qmc", lambda: (*_G, 0, 64, 4, None, None, 30, _ST()), "null pointer"),
    ("olmc_european_qmc", lambda: (*_G, 0, 64, 4, *_sobol(4), 32, _ST()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_european_qmc", lambda: (*_G, 0, 64, 0, *_sobol(1), 30, _ST()), "dims must be in [1, 21201]"),
    ("olmc_european_qmc", lambda: (*_G, 1 << 30, 1, 1, *_sobol(1), 30, _ST()), "at most 2**30 Sobol points"),
    ("olmc_european_qmc", lambda: (*_G, 0, 0, 4, *_sobol(4), 30, _ST()), "n_paths must be >= 1"),
    ("olmc_european_qmc_cv", lambda: (*_G, 0, 64, 4, *_sobol(4), 30, None), "null pointer"),
    ("olmc_european_qmc_cv", lambda: (*_G, -64, 64, 4, *_sobol(4), 30, _CV()), "path_offset must be >= 0"),
    ("olmc_european_qmc_terminal", lambda: (*_MKT, 0, 64, 4, *_sobol(4), 30, 0, None), "null pointer"),
    ("olmc_european_qmc_terminal", lambda: (*_MKT, 0, 64, 4, *_sobol(4), 29, 0, (C.c_double * 64)()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_european_qmc_batch", lambda: (_opts(2), 0, 0, 64, 4, *_sobol(4), 30, (_hip.Stats * 16)()), "batch size must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_european_qmc_batch", lambda: (_opts(2), 2, 0, 64, 4, *_sobol(4), 30, None), "null pointer"),
    ("olmc_european_qmc_batch", lambda: (_opts(2), 2, 0, 64, 22000, *_sobol(4), 30, (_hip.Stats * 16)()), "dims must be in [1, 21201]"),
    ("olmc_european_qmc_greeks_fd", lambda: (*_GT0, 64, 4, *_sobol(4), 30, 0, _out9(), None), "T must be > 0 (price() returns intrinsic value without simulating)"),
    ("olmc_european_qmc_greeks_fd", lambda: (*_G, 64, 4, *_sobol(4), 30, 0, None, None), "null pointer"),
    ("olmc_european_qmc_greeks_fd", lambda: (*_G, 0, 4, *_sobol(4), 30, 0, _out9(), None), "n_paths must be >= 1"),
    ("olmc_asian_qmc", lambda: (*_G, 2, 0, 0, 64, 4, *_sobol(4), 30, 0, _ST()), "bad avg_kind (arithmetic or geometric)"),
    ("olmc_asian_qmc", lambda: (*_G, 0, 2, 0, 64, 4, *_sobol(4), 30, 0, _ST()), "bad construction"),
    ("olmc_asian_qmc", lambda: (*_G, 0, 1, 0, 64, 1025, *_sobol(1025), 30, 0, _ST()),
     "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates"),
    ("olmc_asian_qmc", lambda: (*_G, 0, 0, 0, 64, 4, *_sobol(4), 30, 0, None), "null pointer"),
    ("olmc_asian_qmc", lambda: (*_G, 1, 0, 0, 64, 4, *_sobol(4), 31, 0, _ST()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_extrema_qmc", lambda: (*_G, 6, 120.0, 0, 0, 64, 4, *_sobol(4), 30, 0, _ST()), "bad payoff"),
    ("olmc_extrema_qmc", lambda: (*_G, 1, -2.0, 0, 0, 64, 4, *_sobol(4), 30, 0, _ST()), "Barrier must be positive"),
    ("olmc_extrema_qmc", lambda: (*_G, 4, 0.0, 3, 0, 64, 4, *_sobol(4), 30, 0, _ST()), "bad construction"),
    ("olmc_extrema_qmc", lambda: (*_G, 5, 0.0, 0, 0, 0, 4, *_sobol(4), 30, 0, _ST()), "n_paths must be >= 1"),
    ("olmc_multi_gpu_european", lambda: (*_G, 100, 4, 1, 1, 1, None), "null pointer"),
    ("olmc_multi_gpu_european", lambda: (*_G, 100, 4, 1, 1, 0, _ST()), "n_gpus out of range"),
    ("olmc_multi_gpu_european", lambda: (*_G, 100, 0, 1, 1, 1, _ST()), "n_steps must be >= 1"),
    ("olmc_multi_gpu_european", lambda: (*_G, 3, 4, 1, 1, 4, _ST()), "fewer paths than GPUs"),
    ("olmc_multi_gpu_greeks_fd", lambda: (*_GT0, 100, 4, 1, 0, 1, _out9(), None), "T must be > 0 (price() returns intrinsic value without simulating)"),
    ("olmc_multi_gpu_greeks_fd", lambda: (*_G, 100, 4, 1, 0, 17, _out9(), None), "n_gpus out of range"),
    ("olmc_multi_gpu_european_cv", lambda: (*_G, 100, 4, 1, 1, 1, None), "null pointer"),
    ("olmc_multi_gpu_european_qmc", lambda: (*_G, 64, 4, *_sobol(4), 30, 1, None), "null pointer"),
    ("olmc_multi_gpu_european_qmc", lambda: (*_G, 64, 4, *_sobol(4), 16, 1, _ST()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_multi_gpu_european_qmc_greeks_fd", lambda: (*_GT0, 64, 4, *_sobol(4), 30, 0, 1, _out9(), None),
     "T must be > 0 (price() returns intrinsic value without simulating)"),
    ("olmc_multi_gpu_european_qmc_greeks_fd", lambda: (*_G, 64, 4, *_sobol(4), 30, 0, 0, _out9(), None), "n_gpus out of range"),
    ("olmc_multi_gpu_european_qmc_cv", lambda: (*_G, 64, 0, *_sobol(1), 30, 1, _CV()), "dims must be in [1, 21201]"),
    # two faults at once: the refusal is the one of the check that comes first (the entry point's own, then the Sobol call's:
    # construction, bridge cap, tables, bits, dims, points; then the matrix size)
    ("olmc_asian_qmc", lambda: (*_G, 2, 2, 0, 64, 4, *_sobol(4), 30, 0, _ST()), "bad avg_kind (arithmetic or geometric)"),
    ("olmc_asian_qmc", lambda: (*_G, 0, 2, 0, 64, 4, *_sobol(4), 32, 0, _ST()), "bad construction"),
    ("olmc_asian_qmc", lambda: (*_G, 0, 0, 0, 64, 4, *_sobol(4), 32, 0, None), "null pointer"),
    ("olmc_extrema_qmc", lambda: (*_G, 6, 120.0, 0, 0, 64, 4, *_sobol(4), 32, 0, _ST()), "bad payoff"),
    ("olmc_extrema_qmc", lambda: (*_G, 5, 0.0, 0, 0, 0, 4, *_sobol(4), 32, 0, _ST()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_european_qmc", lambda: (*_G, 0, 0, 0, *_sobol(1), 32, _ST()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_european_qmc_greeks_fd", lambda: (*_GT0, 64, 4, *_sobol(4), 32, 0, _out9(), None),
     "T must be > 0 (price() returns intrinsic value without simulating)"),
    ("olmc_european_qmc_batch", lambda: (_opts(2), 0, 0, 64, 4, *_sobol(4), 32, (_hip.Stats * 16)()), "batch size must be in [1, OLMC_MAX_BATCH]"),
    ("olmc_american_lsm_qmc", lambda: (*_G, 2, 64, 4, *_sobol(4), 30, 5, _ST()), "poly_degree must be in [1, 4]"),
    ("olmc_american_lsm_qmc", lambda: (*_G, 2, 10 ** 9, 10, *_sobol(10), 30, 2, _ST()), "bad construction"),
    ("olmc_gbm_qmc_paths", lambda: (*_MKT, 2, 10 ** 9, 10, *_sobol(10), 30, 0, (C.c_double * 4)()), "bad construction"),
    ("olmc_gbm_qmc_paths", lambda: (*_MKT, 0, 10 ** 9, 10, *_sobol(10), 32, 0, (C.c_double * 4)()),
     "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_exercise_boundary_qmc", lambda: (*_G, 0, 10 ** 9, 10, *_sobol(10), 31, (C.c_double * 4)()),
     "only 30-bit Sobol tables (SciPy's default) are supported"),
    ("olmc_multi_gpu_european_qmc", lambda: (*_G, 64, 4, *_sobol(4), 16, 0, _ST()), "only 30-bit Sobol tables (SciPy's default) are supported"),
    # the path matrices: the model (with its step count) before the path count, the path count before the size
    ("olmc_jump_paths", lambda: (*_MKT, 0, 1.0, -0.1, 0.2, 0.0, 0, 0, 1, 0, (C.c_double * 4)()), "n_steps must be >= 1"),
    ("olmc_jump_paths", lambda: (*_MKT, 2, 1.0, -0.1, 0.2, 0.0, 0, 4, 1, 0, (C.c_double * 4)()), "bad jump model"),
    ("olmc_jump_paths", lambda: (*_MKT, 0, 1.0, -0.1, 0.2, 0.0, 0, 4, 1, 0, (C.c_double * 4)()), "n_paths must be >= 1"),
    ("olmc_gbm_paths", lambda: (*_MKT, 0, 0, 1, 0, (C.c_double * 4)()), "n_paths must be >= 1"),
    ("olmc_gbm_paths", lambda: (*_MKT, 10 ** 9, 0, 1, 0, (C.c_double * 4)()), "n_steps must be >= 1"),
]


@pytest.mark.parametrize("name,args,message", _REFUSALS, ids=[f"{n}-{i}" for i, (n, _a, _m) in enumerate(_REFUSALS)])
def test_entry_points_refuse_bad_arguments_before_touching_a_device(library, name, args, message):
    """Each refusal answers OLMC_ERR_ARG (1) with its exact message, ahead of any device work (no device is initialised here)."""
    refused(library, getattr(library, name)(*args()), message)
