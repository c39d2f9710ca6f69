"""AsianOption / BarrierOption / LookbackOption on the device step loop (reference: ExoticOptionBase._generate_paths
+ AsianOption, src/pricing_models/exotic_options.py:28-160, price_asian :558-572).

Same dataclass fields and ``price(n_paths, n_steps, avg_type, option_type)``
signature; the running average lives in registers, no (n_paths, n_steps) matrix
exists.  Like the reference there is no antithetic mirror unless asked for, and
the return value is a ``numpy.float64``.

Additive: ``method="qmc"`` prices every option here (Asian, barrier, lookback, American (LSM), autocallable, cliquet) on scrambled-Sobol
paths (_qmc_tables, include/olmc.h "quasi-Monte Carlo path payoffs", "... structured products" and "... path matrix"), by default with
the Brownian-bridge construction.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Literal, Optional

import numpy as np

from . import _hip
from ._paths import _barrier_kind, _check_barrier, _check_sizes, _result, _seed
from .black_scholes import _ncdf


def _qmc_precision(method: str, precision: str) -> None:
    """The Sobol path kernels price in fp64 only (AsianOption.price, and its fused Greeks)."""
    if method == "qmc" and precision != "fp64":
        raise ValueError("method='qmc' prices in fp64 only")


def _qmc_tables(method: str, path_construction: str, n_paths: int, n_steps: int, seed: Optional[int], dims_per_step: int = 1):
    """(sv, shift, bridge) for method="qmc", None for "pseudo"; every refusal is a ValueError raised before the device is touched.
    dims_per_step: the Sobol dimensions one step takes (2 for Heston's two factors): the tables hold n_steps * dims_per_step."""
    if method not in ("pseudo", "qmc"):
        raise ValueError("method must be 'pseudo' or 'qmc'")
    if path_construction not in ("bridge", "sequential"):
        raise ValueError("path_construction must be 'bridge' or 'sequential'")
    if method == "pseudo":
        return None
    from .monte_carlo import SOBOL_MAX_DIM, sobol_tables

    if n_steps > SOBOL_MAX_DIM // dims_per_step:
        what = "Sobol dimensions" if dims_per_step == 1 else f"{dims_per_step} Sobol dimensions per step"
        raise ValueError(f"method='qmc' takes at most {SOBOL_MAX_DIM // dims_per_step} steps ({what})")
    bridge = path_construction == "bridge"
    if bridge and n_steps > _hip.QMC_BRIDGE_MAX_STEPS:
        raise ValueError(f"path_construction='bridge' takes at most {_hip.QMC_BRIDGE_MAX_STEPS} steps; use 'sequential'")
    if n_paths > 1 << 30:
        raise ValueError("method='qmc' takes at most 2**30 paths (Sobol points)")
    sv, shift = sobol_tables(n_steps * dims_per_step, _seed(seed), n_paths)
    return sv, shift, bridge


def _draws(method: str, path_construction: str, n_paths: int, n_steps: int, seed: Optional[int], dims_per_step: int = 1):
    """(sobol, run): the arguments a binding takes between its contract and its antithetic or layout flag -- on Sobol points
    (True, (n_paths, sv, shift, bridge)), else (False, (n_paths, n_steps, seed)).  The refusals are _qmc_tables'; seed=None draws one
    seed here, so a caller that asks once launches every cut of a surface or scenario set on the same draws."""
    qmc = _qmc_tables(method, path_construction, n_paths, n_steps, seed, dims_per_step)
    if qmc is not None:
        return True, (n_paths, *qmc)
    return False, (n_paths, n_steps, _seed(seed))


@dataclass
class AsianOption:
    S: float
    K: float
    T: float
    r: float
    sigma: float
    q: float = 0.0
    seed: Optional[int] = None

    def price(self, n_paths: int = 100000, n_steps: int = 252,
              avg_type: Literal["arithmetic", "geometric"] = "arithmetic",
              option_type: Literal["call", "put"] = "call", antithetic: bool = False,
              return_error: bool = False, precision: Literal["fp64", "fp32"] = "fp64",
              method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """precision (additive, arithmetic average only): "fp64" = the reference's arithmetic (fp64 cumulative
        log-return, one fp64 exponential per monitoring date, :62-67); "fp32" = the opt-in fast kernel (one
        hardware fp32 exponential per date: ~2e-6 on the price, 1.6x faster).

        method (additive): "pseudo" (default) = the Philox paths of the pseudo-random kernels; "qmc" = scrambled-Sobol paths: the
        option's seed is the scramble seed of scipy.stats.qmc.Sobol(d=n_steps, scramble=True, seed=seed) (None draws one), point k drives
        path k through z = norm.ppf(clip(u, 1e-10, 1 - 1e-10)).  fp64 only; n_steps <= 21201.
        path_construction (read only with method="qmc"): "bridge" (default) = the Brownian bridge in breadth-first order (dimension 0 sets
        the terminal value, the next ones the midpoints: include/olmc.h), at most 1024 dates; "sequential" = dimension t drives date t + 1.
        With method="qmc", antithetic=True also prices the mirrored point -z, and return_error's standard error is the naive per-path
        one: for Sobol points it is not a confidence interval (it overstates the error).
        Refused (ValueError, before the device is touched): an unknown method or path_construction, method="qmc" with
        precision="fp32", n_steps > 21201 with method="qmc", n_steps > 1024 with the bridge."""
        _check_sizes(n_paths, n_steps)
        if precision not in ("fp64", "fp32"):
            raise ValueError("precision must be 'fp64' or 'fp32'")
        _qmc_precision(method, precision)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)      # seed=None: a fresh draw, as the reference's unseeded RandomState (:51-52)
        contract = (self.S, self.K, self.T, self.r, self.sigma, self.q, option_type == "call", avg_type != "arithmetic")
        st = _hip.asian_qmc(*contract, *run, antithetic) if sobol else _hip.asian(*contract, *run, antithetic, fast=precision == "fp32")
        return _result(st, return_error)

    def price_geometric_closed_form(self, option_type: Literal["call", "put"] = "call") -> float:
        """exotic_options.py:133-160"""
        v = self.sigma / math.sqrt(3)
        b = 0.5 * (self.r - self.q - self.sigma**2 / 6)
        d1 = (math.log(self.S / self.K) + (b + 0.5 * v**2) * self.T) / (v * math.sqrt(self.T))
        d2 = d1 - v * math.sqrt(self.T)
        grow, disc = math.exp((b - self.r) * self.T), math.exp(-self.r * self.T)
        if option_type == "call":
            return self.S * grow * _ncdf(d1) - self.K * disc * _ncdf(d2)
        return self.K * disc * _ncdf(-d2) - self.S * grow * _ncdf(-d1)


def reference_barrier_level(S: float, barrier: float, barrier_type: str) -> float:
    """The level to pass to the C ABI so that its decision at t = 0 is the reference's.

    The ABI decides t = 0 in log space: ln(S_0/S_0) = 0 against ln(B/S), so a barrier at the spot counts as crossed
    (include/olmc.h).  The reference monitors its path matrix, whose column 0 is np.exp(np.log(S)) (exotic_options.py:64-67):
    a few ulps above S for some spots (100, 110), below it for others (80, 120), S itself for the rest (90, 95).  Where the
    two rules disagree the level moves one ulp at a time until they agree; a later date reaches within those ulps of the level
    only on a set of measure zero.  NumPy's exponential and libm's differ on some spots, so this is decided here, on the
    reference's own arithmetic, and not in the C host."""
    if not (S > 0.0 and barrier > 0.0):
        return barrier                                                  # invalid inputs are the ABI's to judge
    up = barrier_type.startswith("up")                                  # exotic_options.py:201-204
    s0 = float(np.exp(np.array([np.log(S)]))[0])                        # the reference's column 0
    wanted = (s0 >= barrier) if up else (s0 <= barrier)
    level = float(barrier)
    toward = math.inf if up != wanted else 0.0                          # up: a higher level crosses less; down: more
    for _ in range(16):
        if ((level / S <= 1.0) if up else (level / S >= 1.0)) == wanted:   # sign of ln(level/S) <= or >= the start at 0
            return level
        level = math.nextafter(level, toward)
    raise AssertionError(f"no level near {barrier} reproduces the reference's t = 0 decision at S = {S}")


@dataclass
class BarrierOption:
    """exotic_options.py:163-224: knock-in / knock-out on discrete monitoring dates t = 0..M; at t = 0 the reference's
    np.exp(np.log(S)) is monitored (reference_barrier_level)."""

    S: float
    K: float
    T: float
    r: float
    sigma: float
    q: float = 0.0
    seed: Optional[int] = None
    barrier: float = 0.0

    def price(self, n_paths: int = 100000, n_steps: int = 252,
              barrier_type: Literal["up-and-out", "up-and-in", "down-and-out", "down-and-in"] = "up-and-out",
              option_type: Literal["call", "put"] = "call", antithetic: bool = False, return_error: bool = False,
              method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """method, path_construction (additive): scrambled-Sobol paths, as AsianOption.price."""
        _check_barrier(self.barrier)
        _check_sizes(n_paths, n_steps)
        kind = _barrier_kind(barrier_type)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)
        level = reference_barrier_level(self.S, self.barrier, barrier_type)
        contract = (self.S, self.K, self.T, self.r, self.sigma, self.q, option_type == "call")
        st = _hip.extrema_qmc(*contract, kind, level, *run, antithetic) if sobol else _hip.barrier(*contract, level, kind, *run, antithetic)
        return _result(st, return_error)


@dataclass
class LookbackOption:
    """exotic_options.py:347-401: floating / fixed strike on the discrete path extrema (t = 0 included)."""

    S: float
    K: float
    T: float
    r: float
    sigma: float
    q: float = 0.0
    seed: Optional[int] = None

    def price(self, n_paths: int = 100000, n_steps: int = 252, lookback_type: Literal["floating", "fixed"] = "floating",
              option_type: Literal["call", "put"] = "call", antithetic: bool = False, return_error: bool = False,
              method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """method, path_construction (additive): scrambled-Sobol paths, as AsianOption.price."""
        _check_sizes(n_paths, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)
        contract = (self.S, self.K, self.T, self.r, self.sigma, self.q, option_type == "call")
        fixed = lookback_type != "floating"                 # anything but "floating" is the fixed strike, as the reference's else branch
        if sobol:
            st = _hip.extrema_qmc(*contract, _hip.LOOKBACK_FIXED if fixed else _hip.LOOKBACK_FLOATING, 0.0, *run, antithetic)
        else:
            st = _hip.lookback(*contract, fixed, *run, antithetic)
        return _result(st, return_error)


@dataclass
class AmericanOption:
    """exotic_options.py:227-345: Longstaff-Schwartz least-squares Monte Carlo on stored device paths."""

    S: float
    K: float
    T: float
    r: float
    sigma: float
    q: float = 0.0
    seed: Optional[int] = None

    def price(self, n_paths: int = 50000, n_steps: int = 50, option_type: Literal["call", "put"] = "put",
              poly_degree: int = 3, return_error: bool = False,
              method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """method, path_construction (additive): "qmc" prices on scrambled-Sobol paths, as AsianOption.price (the seed is the scramble
        seed; the standard error is the naive per-path one), with the same regression as the Philox paths (include/olmc.h "quasi-Monte
        Carlo path matrix").  Refused (ValueError, before the device is touched) as there."""
        _check_sizes(n_paths, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)
        contract = (self.S, self.K, self.T, self.r, self.sigma, self.q, option_type == "call")
        if sobol:
            st = _hip.american_lsm_qmc(*contract, *run, poly_degree)
        else:
            st = _hip.american_lsm(*contract, n_paths, n_steps, poly_degree, run[2])         # the seed comes last there
        return _result(st, return_error)

    def early_exercise_boundary(self, n_paths: int = 10000, n_steps: int = 50, option_type: Literal["call", "put"] = "put",
                                method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """exotic_options.py:309-345: (times, boundary): per date the 10th (put) / 90th (call) percentile of the
        in-the-money simulated prices, NaN where none is; selected on the device from the LSM path set.
        method, path_construction (additive): the Sobol path set of price(method="qmc")."""
        _check_sizes(n_paths, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)
        boundary = (_hip.exercise_boundary_qmc if sobol else _hip.exercise_boundary)(self.S, self.K, self.T, self.r, self.sigma, self.q,
                                                                                    option_type == "call", *run)
        return np.linspace(0, self.T, n_steps + 1), boundary


def price_american(S: float, K: float, T: float, r: float, sigma: float, option_type: str = "put", n_paths: int = 50000,
                   seed: int = None) -> float:
    """exotic_options.py:593-606"""
    return AmericanOption(S=S, K=K, T=T, r=r, sigma=sigma, seed=seed).price(n_paths=n_paths, option_type=option_type)


@dataclass
class AutocallableOption:
    """exotic_options.py:404-491 (snowball note; barriers relative to spot; result = fraction of notional).  observation_freq >
    n_steps leaves no observation date (the reference's range(f, M + 1, f) is empty) and every path runs to maturity; the C ABI
    refuses that case, so it is priced with one observation date, on the last step, at a level no path reaches.  The knock-in minimum includes t = 0 in log space, where the reference
    sees np.exp(np.log(S)) / S; that cannot move a price (a loss needs S_T/S < 1, and the minimum is at most S_T/S), so no level
    is adjusted here."""

    S: float
    K: float
    T: float
    r: float
    sigma: float
    q: float = 0.0
    seed: Optional[int] = None
    autocall_barrier: float = 1.0
    coupon_barrier: float = 0.8
    coupon_rate: float = 0.10
    ki_barrier: float = 0.6

    def price(self, n_paths: int = 100000, n_steps: int = 252, observation_freq: int = 21, antithetic: bool = False,
              return_error: bool = False, method: Literal["pseudo", "qmc"] = "pseudo",
              path_construction: Literal["bridge", "sequential"] = "bridge", **kwargs):
        """method, path_construction (additive): scrambled-Sobol paths, as AsianOption.price (the seed is the scramble seed, the
        standard error the naive per-path one; refusals as there).  **kwargs: the ExoticAdapter's option_type, unread."""
        _check_sizes(n_paths, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)
        autocall_barrier = self.autocall_barrier
        if observation_freq > n_steps:                  # no observation date: nothing redeems early (exotic_options.py:442, 448)
            observation_freq, autocall_barrier = n_steps, math.inf
        st = (_hip.autocallable_qmc if sobol else _hip.autocallable)(self.S, self.T, self.r, self.sigma, self.q, autocall_barrier, self.coupon_barrier,
                                                                     self.coupon_rate, self.ki_barrier, observation_freq, *run, antithetic)
        return _result(st, return_error)


@dataclass
class CliquetOption:
    """exotic_options.py:494-554 (ratchet: sum of locally capped/floored period returns, globally clipped)."""

    S: float
    K: float
    T: float
    r: float
    sigma: float
    q: float = 0.0
    seed: Optional[int] = None
    local_cap: float = 0.05
    local_floor: float = -0.05
    global_cap: float = 0.30
    global_floor: float = 0.0

    def price(self, n_paths: int = 100000, n_steps: int = 252, n_periods: int = 12, antithetic: bool = False,
              return_error: bool = False, method: Literal["pseudo", "qmc"] = "pseudo",
              path_construction: Literal["bridge", "sequential"] = "bridge", **kwargs):
        """method, path_construction (additive): scrambled-Sobol paths, as AsianOption.price (the seed is the scramble seed, the
        standard error the naive per-path one; refusals as there).  **kwargs: the ExoticAdapter's option_type, unread."""
        _check_sizes(n_paths, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, self.seed)
        st = (_hip.cliquet_qmc if sobol else _hip.cliquet)(self.S, self.T, self.r, self.sigma, self.q, self.local_cap, self.local_floor,
                                                           self.global_cap, self.global_floor, n_periods, *run, antithetic)
        return _result(st, return_error)


def price_barrier(S: float, K: float, T: float, r: float, sigma: float, barrier: float, barrier_type: str = "up-and-out",
                  option_type: str = "call", n_paths: int = 100000, seed: int = None) -> float:
    """exotic_options.py:575-590"""
    return BarrierOption(S=S, K=K, T=T, r=r, sigma=sigma, barrier=barrier, seed=seed).price(
        n_paths=n_paths, barrier_type=barrier_type, option_type=option_type)


def price_asian(S: float, K: float, T: float, r: float, sigma: float, avg_type: str = "arithmetic",
                option_type: str = "call", n_paths: int = 100000, seed: int = None) -> float:
    return AsianOption(S=S, K=K, T=T, r=r, sigma=sigma, seed=seed).price(
        n_paths=n_paths, avg_type=avg_type, option_type=option_type)
