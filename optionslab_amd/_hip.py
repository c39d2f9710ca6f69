"""ctypes binding of libolmc.so (C ABI: include/olmc.h).

The library is loaded on first use and there is no CPU fallback: if the shared
object is missing, or no HIP device answers, every call raises
``AccelerationError(..., backend="hip")`` (the reference defines that exception
for exactly this, src/exceptions/montecarlo_exceptions.py:105-131).
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .exceptions import AccelerationError

# $OLMC_LIBRARY overrides the in-tree build (A/B measurements of alternative builds)
LIBRARY_PATH = os.environ.get("OLMC_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libolmc.so")
MAX_BATCH = 16
AVG_ARITHMETIC, AVG_GEOMETRIC, AVG_ARITHMETIC_FAST = 0, 1, 2
_U64 = (1 << 64) - 1


class Stats(C.Structure):
    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_int64),
                ("price", C.c_double), ("std_error", C.c_double)]


class Option(C.Structure):
    _fields_ = [("S", C.c_double), ("K", C.c_double), ("T", C.c_double), ("r", C.c_double),
                ("sigma", C.c_double), ("q", C.c_double), ("is_call", C.c_int32), ("reserved", C.c_int32)]


class HestonScenario(C.Structure):
    _fields_ = [("S", C.c_double), ("K", C.c_double), ("T", C.c_double), ("r", C.c_double), ("q", C.c_double),
                ("kappa", C.c_double), ("theta", C.c_double), ("sigma_v", C.c_double), ("rho", C.c_double), ("v0", C.c_double),
                ("is_call", C.c_int32), ("pad", C.c_int32)]


class CvMoments(C.Structure):
    _fields_ = [("sum_d", C.c_double), ("sum_s", C.c_double), ("sum_dd", C.c_double), ("sum_ss", C.c_double),
                ("sum_ds", C.c_double), ("n", C.c_int64), ("value", C.c_double)]


class DevInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 32), ("compute_units", C.c_int32),
                ("clock_mhz", C.c_int32), ("wavefront", C.c_int32), ("device", C.c_int32), ("hbm_bytes", C.c_int64)]


class LvSurface(C.Structure):
    """ollv_surface (include/olmc_local_vol.h): a host table of local volatilities over (tau, x = ln(S_t / S))."""
    _fields_ = [("vol", C.POINTER(C.c_double)), ("n_x", C.c_int32), ("n_t", C.c_int32), ("x_lo", C.c_double), ("x_hi", C.c_double),
                ("t_hi", C.c_double)]


class SabrModel(C.Structure):
    """olsb_model (include/olmc_sabr.h): alpha = sigma_0, beta the CEV exponent, rho the correlation, nu the volatility of volatility."""
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("rho", C.c_double), ("nu", C.c_double)]


class JdModel(C.Structure):
    """oljd_model (include/olmc_jump.h): Merton (a1, a2) = (mu_j, sigma_j), Kou (a1, a2, a3) = (p, eta1, eta2)."""
    _fields_ = [("model", C.c_int32), ("pad", C.c_int32), ("lambda_j", C.c_double), ("a1", C.c_double), ("a2", C.c_double), ("a3", C.c_double)]


class JsScenario(C.Structure):
    """oljs_scenario (include/olmc_jump_scenarios.h): a contract and its jump model, (a1, a2, a3) as JdModel's."""
    _fields_ = [("S", C.c_double), ("K", C.c_double), ("T", C.c_double), ("r", C.c_double), ("sigma", C.c_double), ("q", C.c_double),
                ("is_call", C.c_int32), ("model", C.c_int32), ("lambda_j", C.c_double), ("a1", C.c_double), ("a2", C.c_double), ("a3", C.c_double)]


_D, _I, _I32, _I64, _U64T, _P = C.c_double, C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_void_p
_DP, _U32P, _I32P = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
_STATS, _CV, _OPTIONS, _SCENARIOS = C.POINTER(Stats), C.POINTER(CvMoments), C.POINTER(Option), C.POINTER(HestonScenario)
_byref = C.byref
_Out9 = C.c_double * 9
# the runs of arguments the entry points share, in the headers' order
_SIX = [_D] * 6                                      # S, K, T, r, sigma, q
_HESTON = [_D] * 5                                   # kappa, theta, sigma_v, rho, v0
_RANGE = [_I64, _I64, _I32, _U64T, _I, _STATS]       # path_offset, n_local, n_steps, seed, antithetic, out
_SOBOL = [_I32, _U32P, _U32P, _I32]                  # n_dims (under Heston: n_steps, of two dimensions each), sv, shift, bits
_POINTS = [_I64, _I64] + _SOBOL                      # point_offset, n_points, then the tables
_CELLS = [_DP, _I32P, _I32]                          # strikes, steps, n_cells
_GREEKS = [_DP, _STATS]                              # out9, the 14 evaluations (or NULL)

# name -> (restype, argtypes); must list every symbol include/olmc.h declares
PROTOTYPES = {
    "olmc_abi_version": (_I, []),
    "olmc_init": (_I, [_I]),
    "olmc_shutdown": (_I, []),
    "olmc_last_error": (C.c_char_p, []),
    "olmc_device_info": (_I, [C.POINTER(DevInfo)]),
    "olmc_european": (_I, _SIX + [_I, _I64, _I32, _U64T, _I, _STATS]),
    "olmc_european_shard": (_I, _SIX + [_I] + _RANGE),
    "olmc_european_shard_dev": (_I, _SIX + [_I, _I64, _I64, _I32, _U64T, _I, _P, _P]),
    "olmc_fetch_dev": (_I, [_P, _I32, _P, _DP]),
    "olmc_european_batch": (_I, [_OPTIONS, _I32] + _RANGE),
    "olmc_european_multi": (_I, [_OPTIONS, _U32P, _I64, _I64, _I32, _U64T, _I, _STATS]),
    "olmc_multi_capacity": (_I, [C.POINTER(_I64)]),
    "olmc_contract_layout": (_I, [_OPTIONS, _I32, _I32, _I32P, _I32P, _U32P, _I32P, _DP]),
    "olmc_european_greeks_fd": (_I, _SIX + [_I, _I64, _I32, _U64T, _I] + _GREEKS),
    "olmc_european_terminal": (_I, [_D] * 5 + [_I64, _I32, _U64T, _I, _DP]),
    "olmc_gbm_paths": (_I, [_D] * 5 + [_I64, _I32, _U64T, _I, _DP]),
    "olmc_european_cv": (_I, _SIX + [_I, _I64, _I32, _U64T, _I, _CV]),
    "olmc_european_cv_shard": (_I, _SIX + [_I, _I64, _I64, _I32, _U64T, _I, _CV]),
    "olmc_combine_cv": (_I, [_CV, _I32, _D, _D, _D, _D, _CV]),
    "olmc_european_qmc": (_I, _SIX + [_I] + _POINTS + [_STATS]),
    "olmc_european_qmc_cv": (_I, _SIX + [_I] + _POINTS + [_CV]),
    "olmc_european_qmc_batch": (_I, [_OPTIONS, _I32] + _POINTS + [_STATS]),
    "olmc_european_qmc_greeks_fd": (_I, _SIX + [_I, _I64] + _SOBOL + [_I] + _GREEKS),
    "olmc_european_qmc_terminal": (_I, [_D] * 5 + _POINTS + [_I, _DP]),
    "olmc_asian": (_I, _SIX + [_I, _I] + _RANGE),
    "olmc_asian_qmc": (_I, _SIX + [_I, _I, _I] + _POINTS + [_I, _STATS]),
    "olmc_extrema_qmc": (_I, _SIX + [_I, _I, _D, _I] + _POINTS + [_I, _STATS]),
    "olmc_asian_qmc_greeks_fd": (_I, _SIX + [_I, _I, _I, _I64] + _SOBOL + [_I, _I] + _GREEKS),
    "olmc_extrema_qmc_greeks_fd": (_I, _SIX + [_I, _I, _D, _I, _I64] + _SOBOL + [_I, _I] + _GREEKS),
    "olmc_asian_greeks_fd": (_I, _SIX + [_I, _I, _I64, _I32, _U64T, _I, _I] + _GREEKS),
    "olmc_extrema_greeks_fd": (_I, _SIX + [_I, _I, _D, _I64, _I32, _U64T, _I, _I] + _GREEKS),
    "olmc_barrier": (_I, _SIX + [_I, _D, _I] + _RANGE),
    "olmc_lookback": (_I, _SIX + [_I, _I] + _RANGE),
    "olmc_autocallable": (_I, [_D] * 9 + [_I32] + _RANGE),
    "olmc_cliquet": (_I, [_D] * 9 + [_I32] + _RANGE),
    "olmc_exercise_boundary": (_I, _SIX + [_I, _I64, _I32, _U64T, _DP]),
    "olmc_heston_paths": (_I, [_D] * 4 + _HESTON + [_I64, _I32, _U64T, _I, _DP, _DP]),
    "olmc_jump_paths": (_I, [_D] * 5 + [_I, _D, _D, _D, _D, _I64, _I32, _U64T, _I, _DP]),
    "olmc_american_lsm": (_I, _SIX + [_I, _I64, _I32, _I32, _U64T, _STATS]),
    "olmc_autocallable_qmc": (_I, [_D] * 9 + [_I32, _I] + _POINTS + [_I, _STATS]),
    "olmc_cliquet_qmc": (_I, [_D] * 9 + [_I32, _I] + _POINTS + [_I, _STATS]),
    "olmc_american_lsm_qmc": (_I, _SIX + [_I, _I, _I64] + _SOBOL + [_I32, _STATS]),
    "olmc_exercise_boundary_qmc": (_I, _SIX + [_I, _I, _I64] + _SOBOL + [_DP]),
    "olmc_gbm_qmc_paths": (_I, [_D] * 5 + [_I, _I64] + _SOBOL + [_I, _DP]),
    "olmc_jump_diffusion": (_I, _SIX + [_I, _I, _D, _D, _D, _D, _I64, _I64, _I32, _U64T, _STATS]),
    "olmc_heston": (_I, [_D] * 5 + [_I] + _HESTON + _RANGE),
    "olmc_heston_qmc": (_I, [_D] * 5 + [_I] + _HESTON + [_I] + _POINTS + [_I, _STATS]),
    "olmc_heston_qmc_paths": (_I, [_D] * 4 + _HESTON + [_I, _I64] + _SOBOL + [_I, _DP, _DP]),
    "olmc_heston_path_payoff": (_I, [_D] * 5 + [_I] + _HESTON + [_I, _D] + _RANGE),
    "olmc_heston_qmc_path_payoff": (_I, [_D] * 5 + [_I] + _HESTON + [_I, _D, _I] + _POINTS + [_I, _STATS]),
    "olmc_heston_surface": (_I, [_D] * 4 + [_I] + _HESTON + _CELLS + _RANGE),
    "olmc_heston_qmc_surface": (_I, [_D] * 4 + [_I] + _HESTON + _CELLS + [_I] + _POINTS + [_I, _STATS]),
    "olmc_heston_scenario_layout": (_I, [_SCENARIOS, _I32, _I32P, _I32P]),
    "olmc_heston_scenarios": (_I, [_SCENARIOS, _I32] + _RANGE),
    "olmc_heston_qmc_scenarios": (_I, [_SCENARIOS, _I32, _I] + _POINTS + [_I, _STATS]),
    "olmc_heston_greeks_fd": (_I, _SIX + [_I] + [_D] * 4 + [_I64, _I32, _U64T, _I, _I] + _GREEKS),
    "olmc_heston_qmc_greeks_fd": (_I, _SIX + [_I] + [_D] * 4 + [_I, _I64] + _SOBOL + [_I, _I] + _GREEKS),
    "olmc_heston_qe_surface": (_I, [_D] * 4 + [_I] + _HESTON + _CELLS + _RANGE),
    "olmc_heston_qe_qmc_surface": (_I, [_D] * 4 + [_I] + _HESTON + _CELLS + [_I] + _POINTS + [_I, _STATS]),
    "olmc_heston_qe_paths": (_I, [_D] * 4 + _HESTON + [_I64, _I32, _U64T, _I, _DP, _DP]),
    "olmc_heston_qe_qmc_paths": (_I, [_D] * 4 + _HESTON + [_I, _I64] + _SOBOL + [_I, _DP, _DP]),
    "olmc_heston_autocallable": (_I, [_D] * 4 + _HESTON + [_D] * 4 + [_I32, _I] + _RANGE),
    "olmc_heston_autocallable_qmc": (_I, [_D] * 4 + _HESTON + [_D] * 4 + [_I32, _I, _I] + _POINTS + [_I, _STATS]),
    "olmc_heston_cliquet": (_I, [_D] * 4 + _HESTON + [_D] * 4 + [_I32, _I] + _RANGE),
    "olmc_heston_cliquet_qmc": (_I, [_D] * 4 + _HESTON + [_D] * 4 + [_I32, _I, _I] + _POINTS + [_I, _STATS]),
    "olmc_multi_gpu_european": (_I, _SIX + [_I, _I64, _I32, _U64T, _I, _I, _STATS]),
    "olmc_multi_gpu_greeks_fd": (_I, _SIX + [_I, _I64, _I32, _U64T, _I, _I] + _GREEKS),
    "olmc_multi_gpu_european_cv": (_I, _SIX + [_I, _I64, _I32, _U64T, _I, _I, _CV]),
    "olmc_multi_gpu_european_qmc": (_I, _SIX + [_I, _I64] + _SOBOL + [_I, _STATS]),
    "olmc_multi_gpu_european_qmc_greeks_fd": (_I, _SIX + [_I, _I64] + _SOBOL + [_I, _I] + _GREEKS),
    "olmc_multi_gpu_european_qmc_cv": (_I, _SIX + [_I, _I64] + _SOBOL + [_I, _CV]),
    "olmc_multi_gpu_spans": (_I, [_DP]),
    "olmc_combine_stats": (_I, [_STATS, _I32, _D, _D, _STATS]),
    "olmc_philox_words": (_I, [_U64T, _I64, _I64, _I32, _I32, C.c_uint32, _U32P]),
    "olmc_normals": (_I, [_U64T, _I64, _I64, _I32, C.POINTER(C.c_float)]),
    "olmc_profile_enable": (_I, [_I]),
    "olmc_tune": (_I, [_I, _I]),
    "olmc_profile_reset": (_I, []),
    "olmc_kernel_time": (_I, [C.POINTER(_I64), _DP]),
}

# the same for include/olmc_local_vol.h (its own header and prefix: olmc.h and PROTOTYPES stay as they are)
LV_EUROPEAN = 8
_LVS = C.POINTER(LvSurface)
LV_PROTOTYPES = {
    "ollv_price": (_I, [_D] * 5 + [_I, _LVS, _I, _D] + _RANGE),
    "ollv_paths": (_I, [_D] * 4 + [_LVS, _I64, _I32, _U64T, _I, _DP]),
    "ollv_surface_prices": (_I, [_D] * 4 + [_I, _LVS] + _CELLS + _RANGE),
}

# and for include/olmc_local_vol_qmc.h (prefix olvq_: the two dicts above stay as they are)
LVQ_PROTOTYPES = {
    "olvq_price": (_I, [_D] * 5 + [_I, _LVS, _I, _D, _I] + _POINTS + [_I, _STATS]),
    "olvq_paths": (_I, [_D] * 4 + [_LVS, _I, _I64] + _SOBOL + [_I, _DP]),
    "olvq_surface_prices": (_I, [_D] * 4 + [_I, _LVS] + _CELLS + [_I] + _POINTS + [_I, _STATS]),
}

# and for include/olmc_jump.h (prefix oljd_)
JD_EUROPEAN = 8
_JDM = C.POINTER(JdModel)
JD_PROTOTYPES = {
    "oljd_price": (_I, _SIX + [_I, _JDM, _I, _D] + _RANGE),
    "oljd_surface_prices": (_I, [_D] * 5 + [_I, _JDM] + _CELLS + _RANGE),
    "oljd_autocallable": (_I, [_D] * 5 + [_JDM] + [_D] * 4 + [_I32] + _RANGE),
    "oljd_cliquet": (_I, [_D] * 5 + [_JDM] + [_D] * 4 + [_I32] + _RANGE),
    "oljd_paths": (_I, [_D] * 5 + [_JDM, _I64, _I32, _U64T, _I, _I, _DP]),
}

# and for include/olmc_jump_scenarios.h (prefix oljs_)
_JSS = C.POINTER(JsScenario)
JS_PROTOTYPES = {
    "oljs_layout": (_I, [_JSS, _I32, _I32P, _I32P]),
    "oljs_scenarios": (_I, [_JSS, _I32] + _RANGE),
    "oljs_greeks_fd": (_I, _SIX + [_I, _JDM, _I64, _I32, _U64T, _I, _I] + _GREEKS),
}

# and for include/olmc_sabr.h (prefix olsb_)
SABR_EUROPEAN = 8
STREAM_SABR = 0x53414252           # OLMC_STREAM_SABR: counter word 3 of the SABR paths' Philox blocks
_SBM = C.POINTER(SabrModel)
SABR_PROTOTYPES = {
    "olsb_price": (_I, [_D] * 4 + [_I, _SBM, _I, _D] + _RANGE),
    "olsb_paths": (_I, [_D] * 2 + [_SBM, _I64, _I32, _U64T, _I, _I, _DP, _DP]),
    "olsb_surface_prices": (_I, [_D] * 3 + [_I, _SBM] + _CELLS + _RANGE),
}

# and for include/olmc_sabr_qmc.h (prefix olsq_: SABR_PROTOTYPES stays as it is)
SABRQ_PROTOTYPES = {
    "olsq_price": (_I, [_D] * 4 + [_I, _SBM, _I, _D, _I] + _POINTS + [_I, _STATS]),
    "olsq_paths": (_I, [_D] * 2 + [_SBM, _I, _I64] + _SOBOL + [_I, _I, _DP, _DP]),
    "olsq_surface_prices": (_I, [_D] * 3 + [_I, _SBM] + _CELLS + [_I] + _POINTS + [_I, _STATS]),
}

# and for include/olha.h (prefix olha_)
HA_BASIS_SPOT_VARIANCE, HA_BASIS_SPOT = 0, 1
HA_PROTOTYPES = {
    "olha_american_lsm": (_I, [_D] * 5 + [_I] + _HESTON + [_I, _I, _I32, _I64, _I32, _U64T, _STATS]),
    "olha_american_lsm_qmc": (_I, [_D] * 5 + [_I] + _HESTON + [_I, _I, _I32, _I, _I64, _U32P, _U32P, _I32, _I32, _STATS]),
    "olha_regressor_scales": (_I, [_D] * 5 + [_I] + [_D] * 4 + [_I32] + [_DP] * 4),
}

_lock = threading.Lock()
_lib: Optional[C.CDLL] = None
_initialised = False


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, unversioned soname).  If
    libolmc initialises the system runtime first, a later `import torch` in the same process brings up a
    SECOND runtime and reports "no GPUs found"; with torch's copy loaded globally first, libolmc's HIP symbols
    bind to it (global scope wins) and the process has one runtime whichever is imported first -- needed
    because torch streams / device buffers are handed to olmc_european_shard_dev.  torch itself is NOT
    imported here.  OLMC_SYSTEM_HIP=1 opts out."""
    if "torch" in sys.modules or os.environ.get("OLMC_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library() -> C.CDLL:
    """dlopen libolmc.so and bind every prototype (no device is touched)."""
    global _lib
    with _lock:
        if _lib is None:
            _share_hip_runtime_with_torch()
            if not os.path.exists(LIBRARY_PATH):
                raise AccelerationError(
                    f"{LIBRARY_PATH} is not built (run `python -m optionslab_amd.build`); there is no CPU fallback",
                    backend="hip")
            try:
                lib = C.CDLL(LIBRARY_PATH)
            except OSError as e:
                raise AccelerationError(f"cannot load {LIBRARY_PATH}: {e}", backend="hip") from e
            for name, (res, args) in (list(PROTOTYPES.items()) + list(LV_PROTOTYPES.items()) + list(LVQ_PROTOTYPES.items())
                                      + list(JD_PROTOTYPES.items()) + list(JS_PROTOTYPES.items()) + list(HA_PROTOTYPES.items())
                                      + list(SABR_PROTOTYPES.items()) + list(SABRQ_PROTOTYPES.items())):
                try:
                    fn = getattr(lib, name)
                except AttributeError:
                    if os.environ.get("OLMC_LIBRARY"):      # an older build under A/B measurement: newer entry points are simply absent
                        continue
                    raise AccelerationError(f"{LIBRARY_PATH} lacks {name}: stale build (run `python -m optionslab_amd.build`)", backend="hip")
                fn.restype, fn.argtypes = res, args
            _lib = lib
        return _lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_library().olmc_last_error().decode("utf-8", "replace")
        raise AccelerationError(f"libolmc error {rc}: {msg}", backend="hip")


def lib() -> C.CDLL:
    """Loaded library with the device initialised (device = $OLMC_DEVICE, else $LOCAL_RANK, else 0)."""
    global _initialised
    l = load_library()
    if not _initialised:
        dev = int(os.environ.get("OLMC_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _check(l.olmc_init(dev))
        _initialised = True
    return l


def hip_available() -> bool:
    try:
        lib()
        return True
    except AccelerationError:
        return False


def shutdown() -> None:
    global _initialised
    if _lib is not None:
        _lib.olmc_shutdown()
    _initialised = False


def seed64(seed: int) -> int:
    return int(seed) & _U64


def device_info() -> dict:
    info = DevInfo()
    _check(lib().olmc_device_info(C.byref(info)))
    arch = info.arch.decode()
    return dict(name=info.name.decode() or f"AMD Instinct ({arch.split(':')[0]})", arch=arch, compute_units=info.compute_units,
                clock_mhz=info.clock_mhz, wavefront=info.wavefront, device=info.device, hbm_bytes=info.hbm_bytes)


# ---- the marshalling every wrapper below shares: one spelling per kind of argument and per kind of answer.  european(), the
# want_evals=False branch of european_greeks_fd() and european_multi() do not use it: they are the latency paths bench.py times and are
# written flat on purpose (their comments say what each spares).
def _answer(rc: int, out):
    """Check a call's return code and hand back what the call filled.  `return _answer(entry(..., _byref(out := Stats())), out)` is the
    whole of a wrapper that allocates a Stats or a CvMoments, calls, checks and returns it: one frame, as the written-out form had."""
    if rc:
        _check(rc)
    return out


def _greeks(want_evals: bool, entry, *args) -> Tuple[List[float], List[Stats]]:
    """Call a fused-Greeks entry point, whose last two arguments are the nine values and the fourteen evaluations (NULL unless wanted)."""
    out9 = _Out9()
    evals = (Stats * 14)() if want_evals else None
    _check(entry(*args, out9, evals))
    return list(out9), (list(evals) if want_evals else [])


def _pointer(a: np.ndarray, kind):
    """A POINTER(kind) at the array's first element that keeps the array alive, as ndarray.ctypes.data_as does, without the cast that
    data_as makes of it: a Sobol or surface call asks for two (profiles/r25_binding_marshalling.jsonl, the `pointer` rows)."""
    p = C.POINTER(kind)(kind.from_address(a.ctypes.data))
    p._arr = a
    return p


def _dp(a: np.ndarray):
    return _pointer(a, _D)


def _options(options):
    """(the olmc_option array, k) of contracts (S, K, T, r, sigma, q, is_call)."""
    k = len(options)
    return (Option * k)(*[Option(S, K, T, r, v, q, int(c), 0) for (S, K, T, r, v, q, c) in options]), k


def european(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int, antithetic: bool = True,
             path_offset: int = 0) -> Stats:
    out = Stats()
    rc = lib().olmc_european_shard(S, K, T, r, sigma, q, bool(is_call), int(path_offset), int(n_paths), int(n_steps), int(seed) & _U64,
                                   bool(antithetic), _byref(out))
    if rc:                              # the hot blocking call of price(): no helper frames on the success path
        _check(rc)
    return out


def european_shard_dev(S, K, T, r, sigma, q, is_call: bool, path_offset: int, n_local: int, n_steps: int, seed: int,
                       antithetic: bool, d_triple_ptr: int, stream_ptr: int = 0) -> None:
    _check(lib().olmc_european_shard_dev(S, K, T, r, sigma, q, int(is_call), int(path_offset), int(n_local), int(n_steps),
                                         seed64(seed), int(antithetic), C.c_void_p(d_triple_ptr),
                                         C.c_void_p(stream_ptr) if stream_ptr else None))


def fetch_dev(d_src_ptr: int, n: int, stream_ptr: int = 0) -> List[float]:
    """Blocking fetch of n doubles that work queued on the stream leaves at the device pointer (olmc_fetch_dev)."""
    out = (C.c_double * int(n))()
    _check(lib().olmc_fetch_dev(C.c_void_p(d_src_ptr), int(n), C.c_void_p(stream_ptr) if stream_ptr else None, out))
    return list(out)


def european_batch(options: Sequence[Tuple[float, float, float, float, float, float, bool]], n_paths: int, n_steps: int,
                   seed: int, antithetic: bool = True, path_offset: int = 0) -> List[Stats]:
    arr, k = _options(options)
    out = (Stats * k)()
    _check(lib().olmc_european_batch(arr, k, int(path_offset), int(n_paths), int(n_steps), seed64(seed), int(antithetic), out))
    return list(out)


_OPTION_DT = np.dtype([("S", "f8"), ("K", "f8"), ("T", "f8"), ("r", "f8"), ("sigma", "f8"), ("q", "f8"), ("is_call", "i4"), ("reserved", "i4")])
_STATS_DT = np.dtype([("sum", "f8"), ("sumsq", "f8"), ("n", "i8"), ("price", "f8"), ("std_error", "f8")])
assert _OPTION_DT.itemsize == C.sizeof(Option) == 56 and _STATS_DT.itemsize == C.sizeof(Stats) == 40
_P_OPTION, _P_STATS, _P_U32 = C.POINTER(Option), C.POINTER(Stats), C.POINTER(C.c_uint32)


def european_multi(S, K, T, r, sigma, q, is_call, n_paths: int, n_steps: int, seed: int, antithetic: bool = True,
                   tags=None) -> np.ndarray:
    """Arrays of contracts -> structured result array with fields of olmc_stats (one launch).  The marshalling is on the
    latency path of small batches (it was 33 us of a 69 us one-contract call), hence the prebuilt dtypes and the direct
    field assignments (NumPy broadcasts scalars and arrays alike)."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    opts = np.empty((n, 7))                      # one olmc_option per row: six doubles, then {is_call, reserved} as two int32
    opts[:, 0], opts[:, 1], opts[:, 2], opts[:, 3], opts[:, 4], opts[:, 5] = S, K, T, r, sigma, q
    flags = opts.view(np.int32)
    flags[:, 12] = is_call
    flags[:, 13] = 0
    out = np.empty((n, 5))                       # one olmc_stats per row (the third column is the int64 sample count)
    ptags = None
    if tags is not None:
        tags = np.ascontiguousarray(tags, dtype=np.uint32)
        ptags = C.cast(tags.ctypes.data, _P_U32)
    _check(lib().olmc_european_multi(C.cast(opts.ctypes.data, _P_OPTION), ptags, n, int(n_paths), int(n_steps), int(seed) & _U64,
                                     bool(antithetic), C.cast(out.ctypes.data, _P_STATS)))
    return out.view(_STATS_DT).reshape(n)


def contract_layout(options: Sequence[Tuple[float, float, float, float, float, float, bool]], n_steps: int):
    """(nsets, pos[k], base_mask, upper_continues_slot0, scale[nsets]) of a set of contracts for the fused kernels (olmc_contract_layout;
    pure host function: loads the library, not the GPU)."""
    arr, k = _options(options)
    nsets, pos, mask, cont, scale = C.c_int32(0), (C.c_int32 * k)(), C.c_uint32(0), C.c_int32(0), (C.c_double * 16)()
    _check(load_library().olmc_contract_layout(arr, k, int(n_steps), C.byref(nsets), pos, C.byref(mask), C.byref(cont), scale))
    return nsets.value, list(pos), mask.value, bool(cont.value), list(scale)[:nsets.value]


def multi_capacity() -> Tuple[int, int]:
    """(contracts, workgroups per contract) the batch workspace of european_multi is sized for right now."""
    out = (C.c_int64 * 2)()
    _check(lib().olmc_multi_capacity(out))
    return int(out[0]), int(out[1])


def european_greeks_fd(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int,
                       second_order: bool, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """(price, delta, gamma, vega, theta, rho, vanna, charm, vomma) and -- unless want_evals is False, which spares a blocking
    Greeks call the marshalling of fourteen structs AND lets the library launch its prices-only kernel -- the statistics of the
    bumped contracts in the reference's call order."""
    if want_evals:
        return _greeks(True, lib().olmc_european_greeks_fd, S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps), seed64(seed),
                       int(second_order))
    out9 = _Out9()
    rc = lib().olmc_european_greeks_fd(S, K, T, r, sigma, q, bool(is_call), int(n_paths), int(n_steps), int(seed) & _U64, bool(second_order), out9, None)
    if rc:                              # the hot blocking call of greeks(): no helper frames on the success path
        _check(rc)
    return out9[:], []


def european_terminal(S, T, r, sigma, q, n_paths: int, n_steps: int, seed: int, antithetic: bool = True) -> np.ndarray:
    out = np.empty(int(n_paths) * (2 if antithetic else 1), dtype=np.float64)
    _check(lib().olmc_european_terminal(S, T, r, sigma, q, int(n_paths), int(n_steps), seed64(seed), int(antithetic), _dp(out)))
    return out


def _path_matrix(n_paths: int, n_steps: int, path_major: bool) -> np.ndarray:
    return np.empty((int(n_paths), int(n_steps) + 1) if path_major else (int(n_steps) + 1, int(n_paths)), dtype=np.float64)


def gbm_paths(S, T, r, sigma, q, n_paths: int, n_steps: int, seed: int, path_major: bool = False) -> np.ndarray:
    """Prices at dates 0 .. n_steps (date 0 = spot): (n_steps + 1, n_paths) time-major, or with path_major
    the reference's (n_paths, n_steps + 1) C-order array, written in that layout by the kernel."""
    out = _path_matrix(n_paths, n_steps, path_major)
    _check(lib().olmc_gbm_paths(S, T, r, sigma, q, int(n_paths), int(n_steps), seed64(seed), int(path_major), _dp(out)))
    return out


def _spot_and_variance(entry, n_paths: int, n_steps: int, path_major: bool, *args):
    """Call a Heston path-matrix entry point, whose last three arguments are path_major and the two matrices; layouts as gbm_paths."""
    spot = _path_matrix(n_paths, n_steps, path_major)
    var = np.empty_like(spot)
    _check(entry(*args, int(path_major), _dp(spot), _dp(var)))
    return spot, var


def heston_paths(S, T, r, q, kappa, theta, sigma_v, rho, v0, n_paths: int, n_steps: int, seed: int, path_major: bool = False):
    """Spot and variance at dates 0 .. n_steps (date 0 = (S, v0)); layouts as gbm_paths."""
    return _spot_and_variance(lib().olmc_heston_paths, n_paths, n_steps, path_major, S, T, r, q, kappa, theta, sigma_v, rho, v0, int(n_paths),
                              int(n_steps), seed64(seed))


def jump_paths(S, T, r, sigma, q, kou: bool, lambda_j, a1, a2, a3, n_paths: int, n_steps: int, seed: int,
               path_major: bool = False) -> np.ndarray:
    """Prices of the jump-diffusion recursion at dates 0 .. n_steps (date 0 = spot); layouts as gbm_paths."""
    out = _path_matrix(n_paths, n_steps, path_major)
    _check(lib().olmc_jump_paths(S, T, r, sigma, q, int(bool(kou)), lambda_j, a1, a2, a3, int(n_paths), int(n_steps), seed64(seed),
                                 int(path_major), _dp(out)))
    return out


def exercise_boundary(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int) -> np.ndarray:
    out = np.empty(int(n_steps) + 1, dtype=np.float64)
    _check(lib().olmc_exercise_boundary(S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps), seed64(seed), _dp(out)))
    return out


def european_cv(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int,
                antithetic: bool = True) -> CvMoments:
    return _answer(lib().olmc_european_cv(S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps),
                                          seed64(seed), int(antithetic), _byref(out := CvMoments())), out)


def european_cv_shard(S, K, T, r, sigma, q, is_call: bool, path_offset: int, n_local: int, n_steps: int, seed: int,
                      antithetic: bool = True) -> CvMoments:
    return _answer(lib().olmc_european_cv_shard(S, K, T, r, sigma, q, int(is_call), int(path_offset), int(n_local), int(n_steps),
                                                seed64(seed), int(antithetic), _byref(out := CvMoments())), out)


def combine_cv(parts, S, T, r, q) -> CvMoments:
    """Control-variate estimate from per-shard moments (pure host function; loads the library, not the GPU)."""
    arr = (CvMoments * len(parts))(*parts)
    return _answer(load_library().olmc_combine_cv(arr, len(parts), S, T, r, q, _byref(out := CvMoments())), out)


def _u32(a: np.ndarray):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, _pointer(a, C.c_uint32)


class _SobolTables:
    """A Sobol call's tables as one value, as the C host carries them: it keeps sv and shift alive for the call and holds `steps`
    (dims / dims_per_step) and `run`, the (steps, sv, shift, bits) run of arguments every Sobol entry point takes."""
    __slots__ = ("sv", "shift", "steps", "run")

    def __init__(self, sv, shift, dims_per_step: int):
        self.sv, psv = _u32(sv)
        self.shift, psh = _u32(shift)
        dims = int(self.sv.shape[0])
        if dims % dims_per_step:
            raise ValueError("Heston takes two Sobol dimensions per step: the tables must hold an even number of dimensions" if dims_per_step == 2
                             else f"the tables must hold a multiple of {dims_per_step} Sobol dimensions")
        self.steps = dims // dims_per_step
        self.run = (self.steps, psv, psh, int(self.sv.shape[1]))


def _sobol_args(sv, shift, point_offset: int, n_paths: int, dims_per_step: int = 1) -> _SobolTables:
    """The tables as C pointers -- after checking that the point range lies inside the columns the table KNOWS: tables derived from
    the engine's public behaviour (monte_carlo.SobolDirections.valid_bits < 30) hold zeros beyond, and a point index there would
    silently repeat earlier points.  Plain arrays count as complete (30 bits).  dims_per_step: the dimensions one step takes (2 under
    Heston, whose entry points take the number of steps where the others take the number of dimensions)."""
    bits = int(getattr(sv, "valid_bits", 30))
    if int(point_offset) + int(n_paths) > (1 << bits):
        raise ValueError(f"Sobol points [{int(point_offset)}, {int(point_offset) + int(n_paths)}) reach beyond the 2**{bits} points these tables were "
                         f"derived for: ask sobol_tables(n_steps, seed, n_points=point_offset + n_paths)")
    return _SobolTables(sv, shift, dims_per_step)


def european_qmc(S, K, T, r, sigma, q, is_call: bool, n_paths: int, sv: np.ndarray, shift: np.ndarray,
                 point_offset: int = 0) -> Stats:
    """sv: (dims, 30) uint32 scrambled direction matrix, shift: (dims,) uint32 (see olmc.h)."""
    sobol = _sobol_args(sv, shift, point_offset, n_paths)
    return _answer(lib().olmc_european_qmc(S, K, T, r, sigma, q, int(is_call), int(point_offset), int(n_paths), *sobol.run, _byref(out := Stats())), out)


def european_qmc_cv(S, K, T, r, sigma, q, is_call: bool, n_paths: int, sv: np.ndarray, shift: np.ndarray, point_offset: int = 0) -> CvMoments:
    sobol = _sobol_args(sv, shift, point_offset, n_paths)
    return _answer(lib().olmc_european_qmc_cv(S, K, T, r, sigma, q, int(is_call), int(point_offset),
                                              int(n_paths), *sobol.run, _byref(out := CvMoments())), out)


def european_qmc_batch(options: Sequence[Tuple[float, float, float, float, float, float, bool]], n_paths: int, sv: np.ndarray, shift: np.ndarray,
                       point_offset: int = 0) -> List[Stats]:
    """k <= 16 contracts (S, K, T, r, sigma, q, is_call) on the same Sobol points, one launch (olmc_european_qmc_batch)."""
    sobol = _sobol_args(sv, shift, point_offset, n_paths)
    arr, k = _options(options)
    out = (Stats * k)()
    _check(lib().olmc_european_qmc_batch(arr, k, int(point_offset), int(n_paths), *sobol.run, out))
    return list(out)


def european_qmc_greeks_fd(S, K, T, r, sigma, q, is_call: bool, n_paths: int, sv: np.ndarray, shift: np.ndarray, second_order: bool,
                           want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As european_greeks_fd, on the Sobol points of a MCMethod.QMC pricer: the 8 / 14 bumped contracts in ONE launch."""
    sobol = _sobol_args(sv, shift, 0, n_paths)
    return _greeks(want_evals, lib().olmc_european_qmc_greeks_fd, S, K, T, r, sigma, q, int(is_call), int(n_paths), *sobol.run, int(second_order))


def european_qmc_terminal(S, T, r, sigma, q, n_paths: int, sv: np.ndarray, shift: np.ndarray,
                          point_offset: int = 0, antithetic: bool = False) -> np.ndarray:
    sobol = _sobol_args(sv, shift, point_offset, n_paths)
    out = np.empty(int(n_paths) * (2 if antithetic else 1), dtype=np.float64)
    _check(lib().olmc_european_qmc_terminal(S, T, r, sigma, q, int(point_offset), int(n_paths), *sobol.run, int(antithetic), _dp(out)))
    return out


def asian(S, K, T, r, sigma, q, is_call: bool, geometric: bool, n_paths: int, n_steps: int, seed: int,
          antithetic: bool = False, path_offset: int = 0, fast: bool = False) -> Stats:
    """fast=True (arithmetic only): the fp32-exponent kernel (OLMC_AVG_ARITHMETIC_FAST); default = reference precision."""
    kind = AVG_GEOMETRIC if geometric else (AVG_ARITHMETIC_FAST if fast else AVG_ARITHMETIC)
    return _answer(lib().olmc_asian(S, K, T, r, sigma, q, int(is_call), kind, int(path_offset), int(n_paths), int(n_steps),
                                    seed64(seed), int(antithetic), _byref(out := Stats())), out)


def _average(geometric: bool) -> int:
    return AVG_GEOMETRIC if geometric else AVG_ARITHMETIC


def asian_greeks_fd(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int, antithetic: bool, second_order: bool,
                    want_evals: bool = True, geometric: bool = False) -> Tuple[List[float], List[Stats]]:
    """As european_greeks_fd for the Asian option (arithmetic at the reference's precision, or geometric): the 8 / 14 bumped contracts in
    ONE launch."""
    return _greeks(want_evals, lib().olmc_asian_greeks_fd, S, K, T, r, sigma, q, int(is_call), _average(geometric), int(n_paths), int(n_steps),
                   seed64(seed), int(antithetic), int(second_order))


LOOKBACK_FLOATING, LOOKBACK_FIXED = 4, 5
PATH_ASIAN_ARITHMETIC, PATH_ASIAN_GEOMETRIC = 6, 7          # OLMC_PATH_ASIAN_*: continue BARRIER_KINDS (0-3) and LOOKBACK_* (4-5)
QMC_SEQUENTIAL, QMC_BRIDGE = 0, 1
QMC_BRIDGE_MAX_STEPS = 1024          # OLMC_QMC_BRIDGE_MAX_STEPS


def _construction(bridge: bool) -> int:
    return QMC_BRIDGE if bridge else QMC_SEQUENTIAL


def asian_qmc(S, K, T, r, sigma, q, is_call: bool, geometric: bool, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True,
              antithetic: bool = False, point_offset: int = 0) -> Stats:
    """The Asian option on scrambled-Sobol paths (olmc_asian_qmc): n_steps = sv.shape[0] dates, bridge or sequential construction."""
    sobol = _sobol_args(sv, shift, point_offset, n_points)
    return _answer(lib().olmc_asian_qmc(S, K, T, r, sigma, q, int(is_call), _average(geometric), _construction(bridge), int(point_offset), int(n_points),
                                        *sobol.run, int(antithetic), _byref(out := Stats())), out)


def extrema_qmc(S, K, T, r, sigma, q, is_call: bool, payoff: int, level: float, n_points: int, sv: np.ndarray, shift: np.ndarray,
                bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """A barrier (payoff = BARRIER_KINDS value, `level` from reference_barrier_level) or lookback (LOOKBACK_FLOATING / LOOKBACK_FIXED)
    option on scrambled-Sobol paths (olmc_extrema_qmc)."""
    sobol = _sobol_args(sv, shift, point_offset, n_points)
    return _answer(lib().olmc_extrema_qmc(S, K, T, r, sigma, q, int(is_call), int(payoff), float(level), _construction(bridge), int(point_offset),
                                          int(n_points), *sobol.run, int(antithetic), _byref(out := Stats())), out)


def asian_qmc_greeks_fd(S, K, T, r, sigma, q, is_call: bool, geometric: bool, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool,
                        antithetic: bool, second_order: bool, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As asian_greeks_fd on the Sobol points of asian_qmc: the 8 / 14 bumped contracts in ONE launch (olmc_asian_qmc_greeks_fd)."""
    sobol = _sobol_args(sv, shift, 0, n_points)
    return _greeks(want_evals, lib().olmc_asian_qmc_greeks_fd, S, K, T, r, sigma, q, int(is_call), _average(geometric), _construction(bridge),
                   int(n_points), *sobol.run, int(antithetic), int(second_order))


def extrema_qmc_greeks_fd(S, K, T, r, sigma, q, is_call: bool, payoff: int, level: float, n_points: int, sv: np.ndarray, shift: np.ndarray,
                          bridge: bool, antithetic: bool, second_order: bool, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As extrema_greeks_fd on the Sobol points of extrema_qmc: ONE launch (olmc_extrema_qmc_greeks_fd); `level` is every contract's."""
    sobol = _sobol_args(sv, shift, 0, n_points)
    return _greeks(want_evals, lib().olmc_extrema_qmc_greeks_fd, S, K, T, r, sigma, q, int(is_call), int(payoff), float(level), _construction(bridge),
                   int(n_points), *sobol.run, int(antithetic), int(second_order))


def extrema_greeks_fd(S, K, T, r, sigma, q, is_call: bool, payoff: int, barrier: float, n_paths: int, n_steps: int, seed: int, antithetic: bool,
                      second_order: bool, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As european_greeks_fd for a barrier (payoff = BARRIER_KINDS value) or lookback (LOOKBACK_FLOATING / LOOKBACK_FIXED) option: ONE launch."""
    return _greeks(want_evals, lib().olmc_extrema_greeks_fd, S, K, T, r, sigma, q, int(is_call), int(payoff), float(barrier), int(n_paths),
                   int(n_steps), seed64(seed), int(antithetic), int(second_order))


BARRIER_KINDS = {"up-and-out": 0, "up-and-in": 1, "down-and-out": 2, "down-and-in": 3}


def barrier(S, K, T, r, sigma, q, is_call: bool, level: float, kind: int, n_paths: int, n_steps: int, seed: int,
            antithetic: bool = False, path_offset: int = 0) -> Stats:
    return _answer(lib().olmc_barrier(S, K, T, r, sigma, q, int(is_call), float(level), int(kind), int(path_offset), int(n_paths), int(n_steps),
                                      seed64(seed), int(antithetic), _byref(out := Stats())), out)


def lookback(S, K, T, r, sigma, q, is_call: bool, fixed_strike: bool, n_paths: int, n_steps: int, seed: int,
             antithetic: bool = False, path_offset: int = 0) -> Stats:
    return _answer(lib().olmc_lookback(S, K, T, r, sigma, q, int(is_call), int(fixed_strike), int(path_offset), int(n_paths), int(n_steps),
                                       seed64(seed), int(antithetic), _byref(out := Stats())), out)


def autocallable(S, T, r, sigma, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq: int,
                 n_paths: int, n_steps: int, seed: int, antithetic: bool = False, path_offset: int = 0) -> Stats:
    return _answer(lib().olmc_autocallable(S, T, r, sigma, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, int(observation_freq),
                                           int(path_offset), int(n_paths), int(n_steps), seed64(seed), int(antithetic), _byref(out := Stats())), out)


def cliquet(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor, n_periods: int, n_paths: int, n_steps: int,
            seed: int, antithetic: bool = False, path_offset: int = 0) -> Stats:
    return _answer(lib().olmc_cliquet(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor, int(n_periods), int(path_offset), int(n_paths),
                                      int(n_steps), seed64(seed), int(antithetic), _byref(out := Stats())), out)


def autocallable_qmc(S, T, r, sigma, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq: int, n_points: int,
                     sv: np.ndarray, shift: np.ndarray, bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """The autocallable on scrambled-Sobol paths (olmc_autocallable_qmc): n_steps = sv.shape[0] dates, bridge or sequential construction."""
    sobol = _sobol_args(sv, shift, point_offset, n_points)
    return _answer(lib().olmc_autocallable_qmc(S, T, r, sigma, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, int(observation_freq),
                                               _construction(bridge), int(point_offset), int(n_points),
                                               *sobol.run, int(antithetic), _byref(out := Stats())), out)


def cliquet_qmc(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor, n_periods: int, n_points: int, sv: np.ndarray,
                shift: np.ndarray, bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """The cliquet on scrambled-Sobol paths (olmc_cliquet_qmc): n_steps = sv.shape[0] dates, bridge or sequential construction."""
    sobol = _sobol_args(sv, shift, point_offset, n_points)
    return _answer(lib().olmc_cliquet_qmc(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor, int(n_periods), _construction(bridge),
                                          int(point_offset), int(n_points), *sobol.run, int(antithetic), _byref(out := Stats())), out)


def american_lsm(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, poly_degree: int, seed: int) -> Stats:
    return _answer(lib().olmc_american_lsm(S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps),
                                           int(poly_degree), seed64(seed), _byref(out := Stats())), out)


def american_lsm_qmc(S, K, T, r, sigma, q, is_call: bool, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool, poly_degree: int) -> Stats:
    """The American option (LSM) on scrambled-Sobol paths (olmc_american_lsm_qmc): n_steps = sv.shape[0] dates, points [0, n_points)."""
    sobol = _sobol_args(sv, shift, 0, n_points)
    return _answer(lib().olmc_american_lsm_qmc(S, K, T, r, sigma, q, int(is_call), _construction(bridge), int(n_points),
                                               *sobol.run, int(poly_degree), _byref(out := Stats())), out)


def exercise_boundary_qmc(S, K, T, r, sigma, q, is_call: bool, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool) -> np.ndarray:
    """exercise_boundary on the Sobol matrix of american_lsm_qmc (olmc_exercise_boundary_qmc)."""
    sobol = _sobol_args(sv, shift, 0, n_points)
    out = np.empty(sobol.steps + 1, dtype=np.float64)
    _check(lib().olmc_exercise_boundary_qmc(S, K, T, r, sigma, q, int(is_call), _construction(bridge), int(n_points), *sobol.run, _dp(out)))
    return out


def gbm_qmc_paths(S, T, r, sigma, q, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True, path_major: bool = False) -> np.ndarray:
    """Sobol-path prices at dates 0 .. n_steps = sv.shape[0] (date 0 = spot), layouts as gbm_paths (olmc_gbm_qmc_paths)."""
    sobol = _sobol_args(sv, shift, 0, n_points)
    out = _path_matrix(n_points, sobol.steps, path_major)
    _check(lib().olmc_gbm_qmc_paths(S, T, r, sigma, q, _construction(bridge), int(n_points), *sobol.run, int(path_major), _dp(out)))
    return out


def jump_diffusion(S, K, T, r, sigma, q, is_call: bool, kou: bool, lambda_j, a1, a2, a3, n_paths: int, n_steps: int, seed: int,
                   path_offset: int = 0) -> Stats:
    """Merton: (a1, a2) = (mu_j, sigma_j), a3 ignored; Kou: (a1, a2, a3) = (p, eta1, eta2)."""
    return _answer(lib().olmc_jump_diffusion(S, K, T, r, sigma, q, int(is_call), int(kou), lambda_j, a1, a2, a3, int(path_offset), int(n_paths),
                                             int(n_steps), seed64(seed), _byref(out := Stats())), out)


def heston(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, n_paths: int, n_steps: int, seed: int,
           antithetic: bool = False, path_offset: int = 0) -> Stats:
    return _answer(lib().olmc_heston(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, int(path_offset), int(n_paths), int(n_steps),
                                     seed64(seed), int(antithetic), _byref(out := Stats())), out)


def heston_qmc(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, n_points: int, sv: np.ndarray, shift: np.ndarray,
               bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """Heston on scrambled-Sobol paths (olmc_heston_qmc): n_steps = sv.shape[0] / 2 steps, bridge or sequential construction."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    return _answer(lib().olmc_heston_qmc(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, _construction(bridge), int(point_offset), int(n_points),
                                         *sobol.run, int(antithetic), _byref(out := Stats())), out)


def heston_qmc_paths(S, T, r, q, kappa, theta, sigma_v, rho, v0, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True,
                     path_major: bool = False):
    """Spot and variance of the Sobol paths at dates 0 .. n_steps = sv.shape[0] / 2, layouts as heston_paths (olmc_heston_qmc_paths)."""
    sobol = _sobol_args(sv, shift, 0, n_points, 2)
    return _spot_and_variance(lib().olmc_heston_qmc_paths, n_points, sobol.steps, path_major, S, T, r, q, kappa, theta, sigma_v, rho, v0,
                              _construction(bridge), int(n_points), *sobol.run)


def heston_path_payoff(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, payoff: int, barrier: float, n_paths: int, n_steps: int,
                       seed: int, antithetic: bool = False, path_offset: int = 0) -> Stats:
    """An Asian (PATH_ASIAN_*), barrier (BARRIER_KINDS value, `barrier` = the level) or lookback (LOOKBACK_*) option on heston()'s paths, one
    launch (olmc_heston_path_payoff); `barrier` is ignored by the other payoffs."""
    return _answer(lib().olmc_heston_path_payoff(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, int(payoff), float(barrier), int(path_offset),
                                                 int(n_paths), int(n_steps), seed64(seed), int(antithetic), _byref(out := Stats())), out)


def heston_qmc_path_payoff(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, payoff: int, barrier: float, n_points: int,
                           sv: np.ndarray, shift: np.ndarray, bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """heston_path_payoff on heston_qmc()'s scrambled-Sobol paths (olmc_heston_qmc_path_payoff): n_steps = sv.shape[0] / 2."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    return _answer(lib().olmc_heston_qmc_path_payoff(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, int(payoff), float(barrier),
                                                     _construction(bridge), int(point_offset), int(n_points),
                                                     *sobol.run, int(antithetic), _byref(out := Stats())), out)


class _SurfaceCells:
    """The cells of a surface call as one value: it keeps the strikes and steps alive and holds `run`, the (strikes, steps, n_cells) run
    of arguments, and `out`, the cells' Stats."""
    __slots__ = ("strikes", "steps", "run", "out")

    def __init__(self, strikes, steps):
        self.strikes = np.ascontiguousarray(strikes, dtype=np.float64)
        self.steps = np.ascontiguousarray(steps, dtype=np.int32)
        if self.strikes.ndim != 1 or self.strikes.shape != self.steps.shape:
            raise ValueError("strikes and steps must be two lists of one length: cell i is (strikes[i], steps[i])")
        self.run = (_dp(self.strikes), _pointer(self.steps, _I32), len(self.strikes))
        self.out = (Stats * max(len(self.strikes), 1))()

    def answer(self, rc: int) -> List[Stats]:
        """Check the return code of a surface call that was given `out`, and return one Stats per cell."""
        if rc:
            _check(rc)
        return list(self.out)[:len(self.strikes)]


def heston_surface(S, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, strikes, steps, n_paths: int, n_steps: int, seed: int,
                   antithetic: bool = False, path_offset: int = 0) -> List[Stats]:
    """European options at the cells (strikes[i], steps[i]) of the time grid dt = T / n_steps on heston()'s paths, one launch
    (olmc_heston_surface): at most 16 cells, in any order; the answers come in the same order."""
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olmc_heston_surface(S, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, *cells.run, int(path_offset), int(n_paths),
                                                  int(n_steps), seed64(seed), int(antithetic), cells.out))


def heston_qmc_surface(S, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, strikes, steps, n_points: int, sv: np.ndarray,
                       shift: np.ndarray, bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> List[Stats]:
    """heston_surface on heston_qmc()'s scrambled-Sobol paths (olmc_heston_qmc_surface): n_steps = sv.shape[0] / 2 steps to T."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olmc_heston_qmc_surface(S, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, *cells.run, _construction(bridge),
                                                      int(point_offset), int(n_points), *sobol.run, int(antithetic), cells.out))


HESTON_MAX_RECURSIONS = 6          # OLMC_HESTON_MAX_RECURSIONS


def lv_surface(vol, x_lo: float, x_hi: float, t_hi: float = 1.0):
    """(LvSurface, the float64 array it points into -- keep it alive as long as the struct) for a table vol[n_t][n_x] (a 1-D table is one
    row).  Shapes and values are checked by the library."""
    vol = np.ascontiguousarray(vol, dtype=np.float64)
    if vol.ndim == 1:
        vol = vol[None, :]
    if vol.ndim != 2:
        raise ValueError("the local-volatility table must be [n_t][n_x]")
    return LvSurface(_dp(vol), vol.shape[1], vol.shape[0], float(x_lo), float(x_hi), float(t_hi)), vol


def lv_price(S, K, T, r, q, is_call: bool, table, payoff: int, barrier: float, n_paths: int, n_steps: int, seed: int, antithetic: bool = False,
             path_offset: int = 0) -> Stats:
    """One payoff (BARRIER_KINDS value, LOOKBACK_*, PATH_ASIAN_* or LV_EUROPEAN) on local-volatility paths, one launch (ollv_price);
    `table` = (vol[n_t][n_x], x_lo, x_hi, t_hi)."""
    surf, _keep = lv_surface(*table)
    return _answer(lib().ollv_price(S, K, T, r, q, int(is_call), _byref(surf), int(payoff), float(barrier), int(path_offset), int(n_paths), int(n_steps),
                                    seed64(seed), int(antithetic), _byref(out := Stats())), out)


def lv_paths(S, T, r, q, table, n_paths: int, n_steps: int, seed: int, path_major: bool = False) -> np.ndarray:
    """The spot matrix of lv_price's paths (ollv_paths), in gbm_paths' layouts."""
    surf, _keep = lv_surface(*table)
    out = _path_matrix(n_paths, n_steps, path_major)
    _check(lib().ollv_paths(S, T, r, q, _byref(surf), int(n_paths), int(n_steps), seed64(seed), int(path_major), _dp(out)))
    return out


def lv_surface_prices(S, T, r, q, is_call: bool, table, strikes, steps, n_paths: int, n_steps: int, seed: int, antithetic: bool = False,
                      path_offset: int = 0) -> List[Stats]:
    """European options at the cells (strikes[i], steps[i]) on lv_price's paths, one launch (ollv_surface_prices): at most 16 cells."""
    surf, _keep = lv_surface(*table)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().ollv_surface_prices(S, T, r, q, int(is_call), _byref(surf), *cells.run, int(path_offset), int(n_paths), int(n_steps),
                                                  seed64(seed), int(antithetic), cells.out))


def lvq_price(S, K, T, r, q, is_call: bool, table, payoff: int, barrier: float, n_points: int, sv: np.ndarray, shift: np.ndarray,
              bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """lv_price on scrambled-Sobol paths (olvq_price): n_steps = sv.shape[0] dimensions, one per step; sv / shift as extrema_qmc."""
    sobol = _sobol_args(sv, shift, point_offset, n_points)
    surf, _keep = lv_surface(*table)
    return _answer(lib().olvq_price(S, K, T, r, q, int(is_call), _byref(surf), int(payoff), float(barrier), _construction(bridge), int(point_offset),
                                    int(n_points), *sobol.run, int(antithetic), _byref(out := Stats())), out)


def lvq_paths(S, T, r, q, table, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True, path_major: bool = False) -> np.ndarray:
    """The spot matrix of lvq_price's points [0, n_points) (olvq_paths; the non-mirrored leg), in gbm_paths' layouts."""
    sobol = _sobol_args(sv, shift, 0, n_points)
    surf, _keep = lv_surface(*table)
    out = _path_matrix(n_points, sobol.steps, path_major)
    _check(lib().olvq_paths(S, T, r, q, _byref(surf), _construction(bridge), int(n_points), *sobol.run, int(path_major), _dp(out)))
    return out


def lvq_surface_prices(S, T, r, q, is_call: bool, table, strikes, steps, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True,
                       antithetic: bool = False, point_offset: int = 0) -> List[Stats]:
    """lv_surface_prices on lvq_price's points (olvq_surface_prices): sv.shape[0] steps to T, at most 16 cells."""
    sobol = _sobol_args(sv, shift, point_offset, n_points)
    surf, _keep = lv_surface(*table)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olvq_surface_prices(S, T, r, q, int(is_call), _byref(surf), *cells.run, _construction(bridge), int(point_offset), int(n_points),
                                                  *sobol.run, int(antithetic), cells.out))


def jd_model(kou: bool, lambda_j, a1, a2, a3=0.0) -> JdModel:
    return JdModel(int(bool(kou)), 0, float(lambda_j), float(a1), float(a2), float(a3))


def jd_price(S, K, T, r, sigma, q, is_call: bool, model, payoff: int, barrier: float, n_paths: int, n_steps: int, seed: int,
             antithetic: bool = False, path_offset: int = 0) -> Stats:
    """One payoff (BARRIER_KINDS value, LOOKBACK_*, PATH_ASIAN_* or JD_EUROPEAN) on jump_paths' paths, one launch (oljd_price);
    `model` = (kou, lambda_j, a1, a2, a3) as jump_diffusion takes them."""
    m = jd_model(*model)
    return _answer(lib().oljd_price(S, K, T, r, sigma, q, int(is_call), _byref(m), int(payoff), float(barrier), int(path_offset), int(n_paths), int(n_steps),
                                    seed64(seed), int(antithetic), _byref(out := Stats())), out)


def jd_surface_prices(S, T, r, sigma, q, is_call: bool, model, strikes, steps, n_paths: int, n_steps: int, seed: int, antithetic: bool = False,
                      path_offset: int = 0) -> List[Stats]:
    """European options at the cells (strikes[i], steps[i]) on jd_price's paths, one launch (oljd_surface_prices): at most 16 cells."""
    m = jd_model(*model)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().oljd_surface_prices(S, T, r, sigma, q, int(is_call), _byref(m), *cells.run, int(path_offset), int(n_paths), int(n_steps),
                                                  seed64(seed), int(antithetic), cells.out))


def jd_autocallable(S, T, r, sigma, q, model, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq: int, n_paths: int,
                    n_steps: int, seed: int, antithetic: bool = False, path_offset: int = 0) -> Stats:
    """autocallable()'s contract on jd_price's paths, one launch (oljd_autocallable)."""
    m = jd_model(*model)
    return _answer(lib().oljd_autocallable(S, T, r, sigma, q, _byref(m), autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, int(observation_freq),
                                           int(path_offset), int(n_paths), int(n_steps), seed64(seed), int(antithetic), _byref(out := Stats())), out)


def jd_cliquet(S, T, r, sigma, q, model, local_cap, local_floor, global_cap, global_floor, n_periods: int, n_paths: int, n_steps: int, seed: int,
               antithetic: bool = False, path_offset: int = 0) -> Stats:
    """cliquet()'s contract on jd_price's paths, one launch (oljd_cliquet)."""
    m = jd_model(*model)
    return _answer(lib().oljd_cliquet(S, T, r, sigma, q, _byref(m), local_cap, local_floor, global_cap, global_floor, int(n_periods), int(path_offset),
                                      int(n_paths), int(n_steps), seed64(seed), int(antithetic), _byref(out := Stats())), out)


def jd_paths(S, T, r, sigma, q, model, n_paths: int, n_steps: int, seed: int, mirror: bool = False, path_major: bool = False) -> np.ndarray:
    """The spot matrix of one leg of jd_price's paths (oljd_paths), in gbm_paths' layouts: mirror=False is jump_paths' matrix."""
    m = jd_model(*model)
    out = _path_matrix(n_paths, n_steps, path_major)
    _check(lib().oljd_paths(S, T, r, sigma, q, _byref(m), int(n_paths), int(n_steps), seed64(seed), int(bool(mirror)), int(path_major), _dp(out)))
    return out


def sabr_model(alpha, beta, rho, nu) -> SabrModel:
    return SabrModel(float(alpha), float(beta), float(rho), float(nu))


def sabr_price(F, K, T, r, is_call: bool, model, payoff: int, barrier: float, n_paths: int, n_steps: int, seed: int, antithetic: bool = False,
               path_offset: int = 0) -> Stats:
    """One payoff (BARRIER_KINDS value, LOOKBACK_*, PATH_ASIAN_* or SABR_EUROPEAN) on SABR paths of the forward, one launch (olsb_price);
    `model` = (alpha, beta, rho, nu)."""
    m = sabr_model(*model)
    return _answer(lib().olsb_price(F, K, T, r, int(is_call), _byref(m), int(payoff), float(barrier), int(path_offset), int(n_paths), int(n_steps),
                                    seed64(seed), int(antithetic), _byref(out := Stats())), out)


def sabr_paths(F, T, model, n_paths: int, n_steps: int, seed: int, mirror: bool = False, path_major: bool = False):
    """Forward and volatility at dates 0 .. n_steps of one leg of sabr_price's paths (olsb_paths; date 0 = (F, alpha)); layouts as
    gbm_paths."""
    m = sabr_model(*model)
    return _spot_and_variance(lib().olsb_paths, n_paths, n_steps, path_major, F, T, _byref(m), int(n_paths), int(n_steps), seed64(seed),
                              int(bool(mirror)))


def sabr_surface_prices(F, T, r, is_call: bool, model, strikes, steps, n_paths: int, n_steps: int, seed: int, antithetic: bool = False,
                        path_offset: int = 0) -> List[Stats]:
    """European options at the cells (strikes[i], steps[i]) on sabr_price's paths, one launch (olsb_surface_prices): at most 16 cells."""
    m = sabr_model(*model)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olsb_surface_prices(F, T, r, int(is_call), _byref(m), *cells.run, int(path_offset), int(n_paths), int(n_steps),
                                                  seed64(seed), int(antithetic), cells.out))


def sabrq_price(F, K, T, r, is_call: bool, model, payoff: int, barrier: float, n_points: int, sv: np.ndarray, shift: np.ndarray,
                bridge: bool = True, antithetic: bool = False, point_offset: int = 0) -> Stats:
    """sabr_price on scrambled-Sobol paths (olsq_price): n_steps = sv.shape[0] / 2 steps, two dimensions each; sv / shift as heston_qmc."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    m = sabr_model(*model)
    return _answer(lib().olsq_price(F, K, T, r, int(is_call), _byref(m), int(payoff), float(barrier), _construction(bridge), int(point_offset),
                                    int(n_points), *sobol.run, int(antithetic), _byref(out := Stats())), out)


def sabrq_paths(F, T, model, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True, mirror: bool = False,
                path_major: bool = False):
    """Forward and volatility at dates 0 .. n_steps = sv.shape[0] / 2 of one leg of sabrq_price's points [0, n_points) (olsq_paths; date
    0 = (F, alpha)); layouts as gbm_paths."""
    sobol = _sobol_args(sv, shift, 0, n_points, 2)
    m = sabr_model(*model)
    return _spot_and_variance(lib().olsq_paths, n_points, sobol.steps, path_major, F, T, _byref(m), _construction(bridge), int(n_points), *sobol.run,
                              int(bool(mirror)))


def sabrq_surface_prices(F, T, r, is_call: bool, model, strikes, steps, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True,
                         antithetic: bool = False, point_offset: int = 0) -> List[Stats]:
    """sabr_surface_prices on sabrq_price's points (olsq_surface_prices): sv.shape[0] / 2 steps to T, at most 16 cells."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    m = sabr_model(*model)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olsq_surface_prices(F, T, r, int(is_call), _byref(m), *cells.run, _construction(bridge), int(point_offset), int(n_points),
                                                  *sobol.run, int(antithetic), cells.out))


def _jd_scenarios(scenarios):
    """(S, K, T, r, sigma, q, is_call, kou, lambda_j, a1, a2, a3) tuples as the C array."""
    k = len(scenarios)
    return (JsScenario * max(k, 1))(*[JsScenario(S, K, T, r, sigma, q, int(bool(c)), int(bool(kou)), lam, a1, a2, a3)
                                      for (S, K, T, r, sigma, q, c, kou, lam, a1, a2, a3) in scenarios]), k


def jd_scenario_layout(scenarios) -> Tuple[int, List[int]]:
    """(n_groups, group[k]) of a list of scenarios (S, K, T, r, sigma, q, is_call, kou, lambda_j, a1, a2, a3): two share a jump group
    exactly when their (kou, lambda_j, T, a1, a2, a3) are equal as doubles (Merton's unread a3 apart), numbered by first appearance
    (oljs_layout; pure host function: loads the library, not the GPU)."""
    arr, k = _jd_scenarios(scenarios)
    n_groups, group = C.c_int32(0), (C.c_int32 * max(k, 1))()
    _check(load_library().oljs_layout(arr, k, C.byref(n_groups), group))
    return n_groups.value, list(group)[:k]


def jd_scenarios(scenarios, n_paths: int, n_steps: int, seed: int, antithetic: bool = False, path_offset: int = 0) -> List[Stats]:
    """European options under k <= 16 scenarios (S, K, T, r, sigma, q, is_call, kou, lambda_j, a1, a2, a3) on ONE walk over
    jump_diffusion()'s draws, one launch (oljs_scenarios); the answers come in the caller's order."""
    arr, k = _jd_scenarios(scenarios)
    out = (Stats * max(k, 1))()
    _check(lib().oljs_scenarios(arr, k, int(path_offset), int(n_paths), int(n_steps), seed64(seed), int(antithetic), out))
    return list(out)[:k]


def jd_greeks_fd(S, K, T, r, sigma, q, is_call: bool, model, n_paths: int, n_steps: int, seed: int, antithetic: bool, second_order: bool,
                 want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As european_greeks_fd under the jump model (kou, lambda_j, a1, a2, a3): the 7 / 8 / 11 / 14 bumped contracts as ONE scenario launch
    of two jump groups (oljs_greeks_fd)."""
    m = jd_model(*model)
    return _greeks(want_evals, lib().oljs_greeks_fd, S, K, T, r, sigma, q, int(is_call), _byref(m), int(n_paths), int(n_steps), seed64(seed),
                   int(antithetic), int(second_order))


def _scenarios(scenarios):
    """(S, K, T, r, q, is_call, kappa, theta, sigma_v, rho, v0) tuples as the C array."""
    k = len(scenarios)
    return (HestonScenario * max(k, 1))(*[HestonScenario(S, K, T, r, q, kappa, theta, sigma_v, rho, v0, int(bool(c)), 0)
                                          for (S, K, T, r, q, c, kappa, theta, sigma_v, rho, v0) in scenarios]), k


def heston_scenario_layout(scenarios) -> Tuple[int, List[int]]:
    """(n_recursions, group[k]) of a list of scenarios (S, K, T, r, q, is_call, kappa, theta, sigma_v, rho, v0): two share a recursion
    exactly when their (T, kappa, theta, sigma_v, rho, v0) are equal as doubles, numbered by first appearance
    (olmc_heston_scenario_layout; pure host function: loads the library, not the GPU)."""
    arr, k = _scenarios(scenarios)
    n_rec, group = C.c_int32(0), (C.c_int32 * max(k, 1))()
    _check(load_library().olmc_heston_scenario_layout(arr, k, C.byref(n_rec), group))
    return n_rec.value, list(group)[:k]


def heston_scenarios(scenarios, n_paths: int, n_steps: int, seed: int, antithetic: bool = False, path_offset: int = 0) -> List[Stats]:
    """European options under k <= 16 scenarios (S, K, T, r, q, is_call, kappa, theta, sigma_v, rho, v0) of at most 6 recursions on ONE
    walk over heston()'s Philox draws, one launch (olmc_heston_scenarios); the answers come in the caller's order."""
    arr, k = _scenarios(scenarios)
    out = (Stats * max(k, 1))()
    _check(lib().olmc_heston_scenarios(arr, k, int(path_offset), int(n_paths), int(n_steps), seed64(seed), int(antithetic), out))
    return list(out)[:k]


def heston_qmc_scenarios(scenarios, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True, antithetic: bool = False,
                         point_offset: int = 0) -> List[Stats]:
    """heston_scenarios on heston_qmc()'s scrambled-Sobol points (olmc_heston_qmc_scenarios): n_steps = sv.shape[0] / 2; one fill of the
    two bridges serves every recursion."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    arr, k = _scenarios(scenarios)
    out = (Stats * max(k, 1))()
    _check(lib().olmc_heston_qmc_scenarios(arr, k, _construction(bridge), int(point_offset), int(n_points), *sobol.run, int(antithetic), out))
    return list(out)[:k]


def heston_greeks_fd(S, K, T, r, sigma, q, is_call: bool, kappa, theta, sigma_v, rho, n_paths: int, n_steps: int, seed: int, antithetic: bool,
                     second_order: bool, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As european_greeks_fd under the Heston model with sigma -> v0 = sigma^2: the 7 / 8 / 11 / 14 bumped contracts as ONE scenario launch
    of four recursions (olmc_heston_greeks_fd)."""
    return _greeks(want_evals, lib().olmc_heston_greeks_fd, S, K, T, r, sigma, q, int(is_call), kappa, theta, sigma_v, rho, int(n_paths),
                   int(n_steps), seed64(seed), int(antithetic), int(second_order))


def heston_qmc_greeks_fd(S, K, T, r, sigma, q, is_call: bool, kappa, theta, sigma_v, rho, n_points: int, sv: np.ndarray, shift: np.ndarray,
                         bridge: bool, antithetic: bool, second_order: bool, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """heston_greeks_fd on the Sobol points of heston_qmc (olmc_heston_qmc_greeks_fd)."""
    sobol = _sobol_args(sv, shift, 0, n_points, 2)
    return _greeks(want_evals, lib().olmc_heston_qmc_greeks_fd, S, K, T, r, sigma, q, int(is_call), kappa, theta, sigma_v, rho,
                   _construction(bridge), int(n_points), *sobol.run, int(antithetic), int(second_order))


STREAM_HESTON_QE = 0x48514500      # OLMC_STREAM_HESTON_QE: counter word 3 of the QE scheme's Philox blocks


def heston_qe_surface(S, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, strikes, steps, n_paths: int, n_steps: int, seed: int,
                      antithetic: bool = False, path_offset: int = 0) -> List[Stats]:
    """heston_surface by the quadratic-exponential scheme (olmc_heston_qe_surface): one Philox block per step, at most 16 cells."""
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olmc_heston_qe_surface(S, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, *cells.run, int(path_offset), int(n_paths),
                                                     int(n_steps), seed64(seed), int(antithetic), cells.out))


def heston_qe_qmc_surface(S, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, strikes, steps, n_points: int, sv: np.ndarray,
                          shift: np.ndarray, bridge: bool = False, antithetic: bool = False, point_offset: int = 0) -> List[Stats]:
    """heston_qe_surface on scrambled-Sobol points (olmc_heston_qe_qmc_surface): n_steps = sv.shape[0] / 2, sequential construction only
    (bridge=True is passed on and refused by the library)."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    cells = _SurfaceCells(strikes, steps)
    return cells.answer(lib().olmc_heston_qe_qmc_surface(S, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, *cells.run, _construction(bridge),
                                                         int(point_offset), int(n_points), *sobol.run, int(antithetic), cells.out))


HESTON_EULER, HESTON_QE = 0, 1      # olmc.h: OLMC_HESTON_EULER / OLMC_HESTON_QE


def _scheme(qe: bool) -> int:
    return HESTON_QE if qe else HESTON_EULER


def heston_autocallable(S, T, r, q, kappa, theta, sigma_v, rho, v0, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier,
                        observation_freq: int, n_paths: int, n_steps: int, seed: int, antithetic: bool = False, path_offset: int = 0,
                        qe: bool = False) -> Stats:
    """The autocallable on heston()'s paths (qe: on heston_qe_surface()'s), one launch (olmc_heston_autocallable)."""
    return _answer(lib().olmc_heston_autocallable(S, T, r, q, kappa, theta, sigma_v, rho, v0, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier,
                                                  int(observation_freq), _scheme(qe), int(path_offset), int(n_paths), int(n_steps),
                                                  seed64(seed), int(antithetic), _byref(out := Stats())), out)


def heston_autocallable_qmc(S, T, r, q, kappa, theta, sigma_v, rho, v0, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier,
                            observation_freq: int, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True,
                            antithetic: bool = False, point_offset: int = 0, qe: bool = False) -> Stats:
    """heston_autocallable on scrambled-Sobol points (olmc_heston_autocallable_qmc): n_steps = sv.shape[0] / 2; qe takes bridge=False only."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    return _answer(lib().olmc_heston_autocallable_qmc(S, T, r, q, kappa, theta, sigma_v, rho, v0, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier,
                                                      int(observation_freq), _scheme(qe), _construction(bridge), int(point_offset), int(n_points),
                                                      *sobol.run, int(antithetic), _byref(out := Stats())), out)


def heston_cliquet(S, T, r, q, kappa, theta, sigma_v, rho, v0, local_cap, local_floor, global_cap, global_floor, n_periods: int,
                   n_paths: int, n_steps: int, seed: int, antithetic: bool = False, path_offset: int = 0, qe: bool = False) -> Stats:
    """The cliquet on heston()'s paths (qe: on heston_qe_surface()'s), one launch (olmc_heston_cliquet)."""
    return _answer(lib().olmc_heston_cliquet(S, T, r, q, kappa, theta, sigma_v, rho, v0, local_cap, local_floor, global_cap, global_floor, int(n_periods),
                                             _scheme(qe), int(path_offset), int(n_paths), int(n_steps),
                                             seed64(seed), int(antithetic), _byref(out := Stats())), out)


def heston_cliquet_qmc(S, T, r, q, kappa, theta, sigma_v, rho, v0, local_cap, local_floor, global_cap, global_floor, n_periods: int,
                       n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = True, antithetic: bool = False,
                       point_offset: int = 0, qe: bool = False) -> Stats:
    """heston_cliquet on scrambled-Sobol points (olmc_heston_cliquet_qmc): n_steps = sv.shape[0] / 2; qe takes bridge=False only."""
    sobol = _sobol_args(sv, shift, point_offset, n_points, 2)
    return _answer(lib().olmc_heston_cliquet_qmc(S, T, r, q, kappa, theta, sigma_v, rho, v0, local_cap, local_floor, global_cap, global_floor, int(n_periods),
                                                 _scheme(qe), _construction(bridge), int(point_offset), int(n_points),
                                                 *sobol.run, int(antithetic), _byref(out := Stats())), out)


def heston_qe_paths(S, T, r, q, kappa, theta, sigma_v, rho, v0, n_paths: int, n_steps: int, seed: int, path_major: bool = False):
    """Spot and variance of heston_qe_surface's paths at dates 0 .. n_steps (date 0 = (S, v0)); layouts as gbm_paths."""
    return _spot_and_variance(lib().olmc_heston_qe_paths, n_paths, n_steps, path_major, S, T, r, q, kappa, theta, sigma_v, rho, v0,
                              int(n_paths), int(n_steps), seed64(seed))


def heston_qe_qmc_paths(S, T, r, q, kappa, theta, sigma_v, rho, v0, n_points: int, sv: np.ndarray, shift: np.ndarray, bridge: bool = False,
                        path_major: bool = False):
    """Spot and variance of heston_qe_qmc_surface's paths at dates 0 .. n_steps = sv.shape[0] / 2 (olmc_heston_qe_qmc_paths)."""
    sobol = _sobol_args(sv, shift, 0, n_points, 2)
    return _spot_and_variance(lib().olmc_heston_qe_qmc_paths, n_points, sobol.steps, path_major, S, T, r, q, kappa, theta, sigma_v, rho, v0,
                              _construction(bridge), int(n_points), *sobol.run)


def _basis(spot_basis: bool) -> int:
    return HA_BASIS_SPOT if spot_basis else HA_BASIS_SPOT_VARIANCE


def heston_american_lsm(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, n_paths: int, n_steps: int, seed: int, poly_degree: int = 2,
                        spot_basis: bool = False, qe: bool = False) -> Stats:
    """The American option (LSM on the state (S_t, v_t); spot_basis: on S_t alone) on heston_paths' matrices (qe: heston_qe_paths'),
    one chain of per-date launches (olha_american_lsm)."""
    return _answer(lib().olha_american_lsm(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, _scheme(qe), _basis(spot_basis), int(poly_degree),
                                           int(n_paths), int(n_steps), seed64(seed), _byref(out := Stats())), out)


def heston_american_lsm_qmc(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, rho, v0, n_points: int, sv: np.ndarray, shift: np.ndarray,
                            bridge: bool = True, poly_degree: int = 2, spot_basis: bool = False, qe: bool = False) -> Stats:
    """heston_american_lsm on heston_qmc_paths' matrices (qe: heston_qe_qmc_paths', bridge=False only): n_steps = sv.shape[0] / 2
    (olha_american_lsm_qmc, which takes the tables' dimensions after the tables)."""
    steps, psv, psh, bits = _sobol_args(sv, shift, 0, n_points, 2).run
    return _answer(lib().olha_american_lsm_qmc(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, rho, v0, _scheme(qe), _basis(spot_basis), int(poly_degree),
                                               _construction(bridge), int(n_points), psv, psh, 2 * steps, bits, _byref(out := Stats())), out)


def heston_american_scales(S, K, T, r, q, is_call: bool, kappa, theta, sigma_v, v0, n_steps: int):
    """(x_centre, x_width, y_centre, y_width), each (n_steps + 1,): the pairs that standardise heston_american_lsm's regressors
    x = (S_t / K - centre) / width and y = (v_t - centre) / width per date (olha_regressor_scales; pure host function: loads the library,
    not the GPU)."""
    out = [np.empty(int(n_steps) + 1 if n_steps >= 1 else 1, dtype=np.float64) for _ in range(4)]
    _check(load_library().olha_regressor_scales(S, K, T, r, q, int(is_call), kappa, theta, sigma_v, v0, int(n_steps), *[_dp(a) for a in out]))
    return tuple(out)


def multi_gpu_european(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int, antithetic: bool,
                       n_gpus: int) -> Stats:
    return _answer(lib().olmc_multi_gpu_european(S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps), seed64(seed),
                                                 int(antithetic), int(n_gpus), _byref(out := Stats())), out)


def multi_gpu_greeks_fd(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int, second_order: bool, n_gpus: int,
                        want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As european_greeks_fd over n_gpus devices of this process: one launch per rank, ONE all-reduce of the 2 nsets + 1 sums."""
    return _greeks(want_evals, lib().olmc_multi_gpu_greeks_fd, S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps), seed64(seed),
                   int(second_order), int(n_gpus))


def multi_gpu_european_cv(S, K, T, r, sigma, q, is_call: bool, n_paths: int, n_steps: int, seed: int, antithetic: bool, n_gpus: int) -> CvMoments:
    return _answer(lib().olmc_multi_gpu_european_cv(S, K, T, r, sigma, q, int(is_call), int(n_paths), int(n_steps), seed64(seed),
                                                    int(antithetic), int(n_gpus), _byref(out := CvMoments())), out)


def multi_gpu_european_qmc(S, K, T, r, sigma, q, is_call: bool, n_paths: int, sv: np.ndarray, shift: np.ndarray, n_gpus: int) -> Stats:
    """As european_qmc over n_gpus devices of this process: rank d prices points [d N / P, (d + 1) N / P), one all-reduce of 3 sums."""
    sobol = _sobol_args(sv, shift, 0, n_paths)
    return _answer(lib().olmc_multi_gpu_european_qmc(S, K, T, r, sigma, q, int(is_call), int(n_paths), *sobol.run, int(n_gpus), _byref(out := Stats())), out)


def multi_gpu_european_qmc_greeks_fd(S, K, T, r, sigma, q, is_call: bool, n_paths: int, sv: np.ndarray, shift: np.ndarray, second_order: bool,
                                     n_gpus: int, want_evals: bool = True) -> Tuple[List[float], List[Stats]]:
    """As european_qmc_greeks_fd over n_gpus devices of this process: every rank prices the 8 / 14 contracts on its block of the
    Sobol points in one launch, one all-reduce of 17 / 33 sums."""
    sobol = _sobol_args(sv, shift, 0, n_paths)
    return _greeks(want_evals, lib().olmc_multi_gpu_european_qmc_greeks_fd, S, K, T, r, sigma, q, int(is_call), int(n_paths), *sobol.run,
                   int(second_order), int(n_gpus))


def multi_gpu_european_qmc_cv(S, K, T, r, sigma, q, is_call: bool, n_paths: int, sv: np.ndarray, shift: np.ndarray, n_gpus: int) -> CvMoments:
    """As european_qmc_cv over n_gpus devices of this process: one all-reduce of the five moments and n."""
    sobol = _sobol_args(sv, shift, 0, n_paths)
    return _answer(lib().olmc_multi_gpu_european_qmc_cv(S, K, T, r, sigma, q, int(is_call), int(n_paths),
                                                        *sobol.run, int(n_gpus), _byref(out := CvMoments())), out)


def multi_gpu_spans() -> dict:
    """Host microseconds of this thread's last multi-GPU call (olmc_multi_gpu_spans)."""
    out = (C.c_double * 8)()
    _check(lib().olmc_multi_gpu_spans(out))
    return dict(zip(("launch_us", "collective_us", "fetch_us", "drain_us", "total_us", "wake_us_max", "rank_launch_us_max", "rank_launch_us_min"), out))


def combine_stats(parts: Sequence[Tuple[float, float, int]], r: float, T: float) -> Stats:
    """Pure host function: needs the library but no device."""
    k = len(parts)
    arr = (Stats * k)(*[Stats(s, ss, int(n), 0.0, 0.0) for (s, ss, n) in parts])
    return _answer(load_library().olmc_combine_stats(arr, k, r, T, _byref(out := Stats())), out)


def philox_words(seed: int, path_offset: int, n_paths: int, block0: int, n_blocks: int, tag: int = 0) -> np.ndarray:
    out = np.empty((int(n_paths), int(n_blocks), 4), dtype=np.uint32)
    _check(lib().olmc_philox_words(seed64(seed), int(path_offset), int(n_paths), int(block0), int(n_blocks), int(tag),
                                   _pointer(out, C.c_uint32)))
    return out


def normals(seed: int, path_offset: int, n_paths: int, n_steps: int) -> np.ndarray:
    out = np.empty((int(n_paths), int(n_steps)), dtype=np.float32)
    _check(lib().olmc_normals(seed64(seed), int(path_offset), int(n_paths), int(n_steps), _pointer(out, C.c_float)))
    return out


TUNE_GRID_CAP = 2
TUNE_QMC_BLOCK = 4
TUNE_SPLIT_TAIL = 7
TUNE_POLL = 8
TUNE_SPLIT_SAT = 9
TUNE_MULTI_LAUNCH = 10
TUNE_STAGED_COPY = 11
TUNE_PHILOX_TABLE = 12


def tune(knob: int, value: int) -> None:
    _check(load_library().olmc_tune(int(knob), int(value)))


def profile_enable(on: bool) -> None:
    _check(lib().olmc_profile_enable(int(on)))


def profile_reset() -> None:
    _check(lib().olmc_profile_reset())


def kernel_time() -> Tuple[int, float]:
    n, ms = C.c_int64(0), C.c_double(0.0)
    _check(lib().olmc_kernel_time(C.byref(n), C.byref(ms)))
    return n.value, ms.value
