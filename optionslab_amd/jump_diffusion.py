"""Merton and Kou jump-diffusion pricers on the device step loop (reference:
src/pricing_models/jump_diffusion.py:38-372).

`price_monte_carlo` runs on the GPU (one Philox block per step: diffusion normal, Poisson
uniform, jump draws).  `MertonJumpDiffusion.price` is the reference's Poisson-weighted
Black-Scholes series (:69-132) -- scalar host arithmetic, the accuracy anchor of the MC.
Additive: Asians, barriers, lookbacks, a strike x maturity surface, the autocallable and the
cliquet on the same paths, one launch each (include/olmc_jump.h; `_JumpPathPayoffs`); what-if scenario sets and the fused
finite-difference Greeks of the Monte Carlo price (include/olmc_jump_scenarios.h; `price_scenarios`, `JumpMCAdapter`).
"""
from __future__ import annotations

import dataclasses
import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Literal, Optional

import numpy as np

from . import _hip
from ._paths import _SURFACE_CELLS, _asian_payoff, _barrier_kind, _check_barrier, _check_sizes, _fill_surface, _lookback_payoff, _result, _seed, _strike_list, _surface_steps
from .black_scholes import _ncdf


class _JumpPathPayoffs:
    """What both models share, written once over `_jd()`: price_monte_carlo, simulate_paths and the path-dependent pricers
    (include/olmc_jump.h), each of which is ONE launch on simulate_paths' paths that stores no path.  Their parameter names, defaults,
    return conventions and refusals are HestonPricer's methods of the same names, without method= / scheme=; sigma stands where price_monte_carlo has it.  antithetic=True also prices the mirror leg of every path (simulate_paths(mirror=True)):
    the diffusion normals negated, the jump counts and sizes shared; the price is then the mean over 2 n_paths samples and the standard
    error the plain one over those samples."""

    def _jd(self):
        """(kou, lambda_j, a1, a2, a3) of the C ABI."""
        raise NotImplementedError

    def price_monte_carlo(self, S, K, T, r, sigma, option_type: Literal["call", "put"] = "call", q: float = 0.0,
                          n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, return_error: bool = False, *,
                          antithetic: bool = False):
        """antithetic=False is olmc_jump_diffusion's launch; True prices the path and its mirror leg (oljd_price, OLJD_EUROPEAN)."""
        _check_sizes(n_paths, n_steps)
        if antithetic:
            st = _hip.jd_price(S, K, T, r, sigma, q, option_type == "call", self._jd(), _hip.JD_EUROPEAN, 0.0, n_paths, n_steps, _seed(seed), True)
        else:
            st = _hip.jump_diffusion(S, K, T, r, sigma, q, option_type == "call", *self._jd(), n_paths, n_steps, _seed(seed))
        return _result(st, return_error)

    def simulate_paths(self, S, T, r, sigma, q: float = 0.0, n_paths: int = 1, n_steps: int = 252,
                       seed: Optional[int] = None, *, mirror: bool = False) -> np.ndarray:
        """(n_paths, n_steps + 1) price paths of price_monte_carlo's recursion for the same seed, column 0 = S (additive for Kou: the
        reference has them for Merton only); mirror=True: the mirror leg of the same paths (the diffusion normals negated, the jumps
        shared)."""
        _check_sizes(n_paths, n_steps)
        if mirror:
            return _hip.jd_paths(S, T, r, sigma, q, self._jd(), n_paths, n_steps, _seed(seed), mirror=True, path_major=True)
        return _hip.jump_paths(S, T, r, sigma, q, *self._jd(), n_paths, n_steps, _seed(seed), path_major=True)

    def _price_path_payoff(self, payoff, barrier, S, K, T, r, sigma, q, option_type, n_paths, n_steps, seed, antithetic, return_error):
        _check_sizes(n_paths, n_steps)
        st = _hip.jd_price(S, K, T, r, sigma, q, option_type == "call", self._jd(), payoff, barrier, n_paths, n_steps, _seed(seed), antithetic)
        return _result(st, return_error)

    def price_asian(self, S: float, K: float, T: float, r: float, sigma: float, q: float = 0.0,
                    option_type: Literal["call", "put"] = "call", avg_type: Literal["arithmetic", "geometric"] = "arithmetic",
                    n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False,
                    return_error: bool = False):
        """max(+-(A - K), 0), A the arithmetic or geometric mean of the spot over dates 1 .. n_steps: what AsianOption.price computes from
        simulate_paths' matrix for the same seed.  Refused (ValueError, before the device is touched): an unknown avg_type, bad counts."""
        return self._price_path_payoff(_asian_payoff(avg_type), 0.0, S, K, T, r, sigma, q, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_barrier(self, S: float, K: float, T: float, r: float, sigma: float, barrier: float, q: float = 0.0,
                      option_type: Literal["call", "put"] = "call",
                      barrier_type: Literal["up-and-out", "up-and-in", "down-and-out", "down-and-in"] = "up-and-out", n_paths: int = 100000,
                      n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False):
        """max(+-(S_n - K), 0) where the barrier, monitored at dates 0 .. n_steps of simulate_paths' matrix (date 0 is S itself), leaves it
        active: what BarrierOption.price computes from that matrix.  barrier_type is read as the reference's class reads it:
        startswith("up") and endswith("out").  After date 0 the kernel decides in log space, so a path within rounding (about 1e-16
        relative) of the level can decide differently from the matrix route.  Also refused: barrier <= 0."""
        _check_barrier(barrier)
        return self._price_path_payoff(_barrier_kind(barrier_type), barrier, S, K, T, r, sigma, q, option_type, n_paths, n_steps, seed, antithetic,
                                       return_error)

    def price_lookback(self, S: float, K: float, T: float, r: float, sigma: float, q: float = 0.0,
                       option_type: Literal["call", "put"] = "call", lookback_type: Literal["floating", "fixed"] = "floating",
                       n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False,
                       return_error: bool = False):
        """The lookback option on the extrema of simulate_paths' matrix over dates 0 .. n_steps (LookbackOption.price): floating call S_n -
        S_min, floating put S_max - S_n, fixed call max(S_max - K, 0), fixed put max(K - S_min, 0).  Also refused: an unknown
        lookback_type."""
        return self._price_path_payoff(_lookback_payoff(lookback_type), 0.0, S, K, T, r, sigma, q, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_surface(self, S: float, strikes, maturities, r: float, sigma: float, q: float = 0.0,
                      option_type: Literal["call", "put"] = "call", n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None,
                      antithetic: bool = False, return_error: bool = False):
        """European prices on a strike x maturity grid from ONE set of paths: a float64 array (len(strikes), len(maturities)); with
        return_error, (prices, std_errors) of that shape.  n_steps is the number of steps to the longest maturity T, and every maturity
        must lie on that grid, as HestonPricer.price_surface requires (same ValueErrors).  Cell (K, T_j) is exp(-r T_j) mean(max(+-(spot[:,
        m_j] - K), 0)) over column m_j of simulate_paths(S, T, r, sigma, q, n_paths, n_steps, seed); more than 16 cells are cut into
        launches of at most 16, and a cell's bits do not depend on the cells it shares a launch with."""
        ks = _strike_list(strikes)
        _check_sizes(n_paths, n_steps)
        T, steps = _surface_steps(maturities, n_steps)
        s = _seed(seed)
        return _fill_surface(ks, steps, lambda cell_k, cell_m: _hip.jd_surface_prices(S, T, r, sigma, q, option_type == "call", self._jd(), cell_k,
                                                                                      cell_m, n_paths, n_steps, s, antithetic), return_error)

    def price_autocallable(self, S: float, T: float, r: float, sigma: float, q: float = 0.0, autocall_barrier: float = 1.0,
                           coupon_barrier: float = 0.8, coupon_rate: float = 0.10, ki_barrier: float = 0.6, observation_freq: int = 21,
                           n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False,
                           return_error: bool = False):
        """The autocallable note, a fraction of notional: what AutocallableOption.price computes from simulate_paths' matrix.  Levels are
        relative to S; observation dates are observation_freq, 2 observation_freq, ... <= n_steps; a payoff is discounted at its own date;
        the knock-in minimum includes date 0.  observation_freq > n_steps is priced as HestonPricer.price_autocallable prices it (one
        observation on the last step at a level no path reaches).  Also refused: observation_freq < 1."""
        _check_sizes(n_paths, n_steps)
        if observation_freq < 1:
            raise ValueError("observation_freq must be >= 1")
        if observation_freq > n_steps:                  # no observation date: nothing redeems early
            observation_freq, autocall_barrier = n_steps, float("inf")
        st = _hip.jd_autocallable(S, T, r, sigma, q, self._jd(), autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq,
                                  n_paths, n_steps, _seed(seed), antithetic)
        return _result(st, return_error)

    def price_cliquet(self, S: float, T: float, r: float, sigma: float, q: float = 0.0, local_cap: float = 0.05, local_floor: float = -0.05,
                      global_cap: float = 0.30, global_floor: float = 0.0, n_periods: int = 12, n_paths: int = 100000, n_steps: int = 252,
                      seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False):
        """exp(-r T) mean(max(clip(sum of clip(period return, local_floor, local_cap), global_floor, global_cap), 0) S) over n_periods
        periods of n_steps // n_periods steps from date 0 (CliquetOption.price on simulate_paths' matrix); trailing dates never enter a
        period and are not drawn.  Also refused: n_periods outside [1, n_steps]."""
        _check_sizes(n_paths, n_steps)
        if n_periods < 1 or n_periods > n_steps:
            raise ValueError("n_periods must be in [1, n_steps]")
        st = _hip.jd_cliquet(S, T, r, sigma, q, self._jd(), local_cap, local_floor, global_cap, global_floor, n_periods, n_paths, n_steps,
                             _seed(seed), antithetic)
        return _result(st, return_error)

    def _scenario_tuples(self, scenarios):
        """price_scenarios' mappings as _hip's tuples (S, K, T, r, sigma, q, is_call, kou, lambda_j, a1, a2, a3), checked."""
        scenarios = list(scenarios)
        if not scenarios:
            raise ValueError("scenarios must not be empty")
        own = [f.name for f in dataclasses.fields(self)]
        out = []
        for i, sc in enumerate(scenarios):
            missing = [key for key in ("S", "K", "T", "r", "sigma") if key not in sc]
            if missing:
                raise ValueError(f"scenario {i} lacks {missing}")
            unknown = sorted(set(sc) - {"S", "K", "T", "r", "sigma", "q", "option_type", *own})
            if unknown:
                raise ValueError(f"scenario {i} has unknown keys {unknown}")
            T = float(sc["T"])
            if T <= 0.0:
                raise ValueError(f"scenario {i}: T must be > 0")
            try:
                model = dataclasses.replace(self, **{key: float(sc[key]) for key in own if key in sc})      # __post_init__'s checks
            except ValueError as e:
                raise ValueError(f"scenario {i}: {e}") from None
            out.append((float(sc["S"]), float(sc["K"]), T, float(sc["r"]), float(sc["sigma"]), float(sc.get("q", 0.0)),
                        sc.get("option_type", "call") == "call", *model._jd()))
        return out

    def price_scenarios(self, scenarios, n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False,
                        return_error: bool = False):
        """European prices under a list of what-if scenarios on COMMON random numbers: a float64 array (len(scenarios),), with
        return_error (prices, std_errors).  A scenario is a mapping with the keys S, K, T, r, sigma and optionally q (0), option_type
        ("call"; anything else prices as a put) and the model's own fields (this instance's where absent): spot, strike, maturity,
        rates, volatility and the jump law may all differ.  Scenario i is price_monte_carlo(S, K, T, r, sigma, option_type, q, n_paths,
        n_steps, seed, antithetic=antithetic) of a model with its fields -- the same draws, the sums to rounding -- but the scenarios
        of a launch share ONE walk over the Philox blocks: the diffusion enters through one sum of normals per path, and scenarios
        whose (lambda_j, T and jump-size parameters) are equal as doubles share a jump sum, the others take one of their own on the
        same Poisson uniforms and size draws.  The list is cut in the caller's order into launches of at most 16 scenarios; a
        scenario's bits depend neither on the cut nor on its neighbours nor on its place.  seed=None draws ONE seed for all launches.
        Refused (ValueError, before the device is touched): bad counts, an empty list, a scenario without S, K, T, r or sigma, with an
        unknown key, with T <= 0, or with model fields the model's own constructor refuses."""
        _check_sizes(n_paths, n_steps)
        tuples = self._scenario_tuples(scenarios)
        s = _seed(seed)
        prices = np.empty(len(tuples), dtype=np.float64)
        errors = np.empty_like(prices)
        for a in range(0, len(tuples), _SURFACE_CELLS):
            for i, st in enumerate(_hip.jd_scenarios(tuples[a:a + _SURFACE_CELLS], n_paths, n_steps, s, antithetic), a):
                prices[i], errors[i] = st.price, st.std_error
        return (prices, errors) if return_error else prices


@dataclass
class MertonJumpDiffusion(_JumpPathPayoffs):
    lambda_j: float
    mu_j: float
    sigma_j: float

    def __post_init__(self):            # :54-59
        if self.lambda_j < 0:
            raise ValueError("lambda_j must be non-negative")
        if self.sigma_j < 0:
            raise ValueError("sigma_j must be non-negative")

    def _jd(self):
        return (False, self.lambda_j, self.mu_j, self.sigma_j, 0.0)

    @property
    def kappa(self) -> float:           # :61-67
        return math.exp(self.mu_j + 0.5 * self.sigma_j**2) - 1

    def price(self, S, K, T, r, sigma, option_type: Literal["call", "put"] = "call", q: float = 0.0, n_terms: int = 50) -> float:
        """Merton's series (:69-132): sum_n Poisson(lambda' T; n) * BS(r_n, sigma_n)."""
        if T <= 0:
            return max(S - K, 0) if option_type == "call" else max(K - S, 0)
        kappa = self.kappa
        lam_p = self.lambda_j * (1 + kappa)
        total = 0.0
        for n in range(n_terms):
            weight = math.exp(-lam_p * T) * (lam_p * T) ** n / math.factorial(n)
            sigma_n = math.sqrt(sigma**2 + n * self.sigma_j**2 / T)
            r_n = r - self.lambda_j * kappa + n * math.log(1 + kappa) / T
            total += weight * self._black_scholes(S, K, T, r_n, sigma_n, option_type, q)
            if weight < 1e-12:          # :128-130 (checked after adding the term)
                break
        return total

    @staticmethod
    def _black_scholes(S, K, T, r, sigma, option_type, q) -> float:     # :134-158
        fwd, strike = S * math.exp(-q * T), K * math.exp(-r * T)
        if sigma <= 0 or T <= 0:
            return max(fwd - strike, 0) if option_type == "call" else max(strike - fwd, 0)
        root = sigma * math.sqrt(T)
        d1 = (math.log(S / K) + (r - q + 0.5 * sigma**2) * T) / root
        d2 = d1 - root
        if option_type == "call":
            return fwd * _ncdf(d1) - strike * _ncdf(d2)
        return strike * _ncdf(-d2) - fwd * _ncdf(-d1)

    def simulate_path(self, S, T, r, sigma, q: float = 0.0, n_steps: int = 252, seed: Optional[int] = None) -> np.ndarray:
        """jump_diffusion.py:227-272: one path with jumps, shape (n_steps + 1,)."""
        return self.simulate_paths(S, T, r, sigma, q, 1, n_steps, seed)[0]


@dataclass
class KouJumpDiffusion(_JumpPathPayoffs):
    lambda_j: float
    p: float
    eta1: float
    eta2: float

    def __post_init__(self):            # :285-291
        if not 0 <= self.p <= 1:
            raise ValueError("p must be in [0, 1]")
        if self.eta1 <= 1:
            raise ValueError("eta1 must be > 1 for finite mean")
        if self.eta2 <= 0:
            raise ValueError("eta2 must be positive")

    def _jd(self):
        return (True, self.lambda_j, self.p, self.eta1, self.eta2)

    @property
    def kappa(self) -> float:           # :293-299
        return self.p * self.eta1 / (self.eta1 - 1) + (1 - self.p) * self.eta2 / (self.eta2 + 1) - 1


class JumpDiffusionAdapter:
    """unified_greeks.py:155-175: PricerProtocol over a jump-diffusion model's series price."""

    def __init__(self, jd_model):
        self.jd = jd_model

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kwargs) -> float:
        return self.jd.price(S, K, T, r, sigma, option_type, q)


class JumpMCAdapter:
    """PricerProtocol over a jump-diffusion model's device Monte Carlo price: ``price`` is the model's price_monte_carlo at the adapter's
    n_paths, n_steps, seed and antithetic, so compute_greeks_unified(adapter, ...) differentiates the price price_monte_carlo gives --
    for Kou as for Merton, where JumpDiffusionAdapter differentiates Merton's series.  seed=None draws one seed at construction: every
    bump sees the same random numbers.  The adapter carries _fused_greeks, so compute_greeks_unified prices the 7 / 8 / 11 / 14 bumped
    contracts as ONE scenario launch of two jump groups (oljs_greeks_fd); fused=False goes the one launch per evaluation way and gives
    the same numbers to rounding.  Refused (ValueError, before the device is touched): bad counts."""

    def __init__(self, model, n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False):
        _check_sizes(n_paths, n_steps)
        self.jd = model
        self.n_paths, self.n_steps, self.antithetic = int(n_paths), int(n_steps), bool(antithetic)
        self.seed = int(_seed(seed))

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kwargs) -> float:
        return self.jd.price_monte_carlo(S, K, T, r, sigma, option_type, q, self.n_paths, self.n_steps, self.seed, antithetic=self.antithetic, **kwargs)

    def _can_fuse(self, pricer_kwargs) -> bool:
        return not pricer_kwargs

    def _fused_greeks(self, S, K, T, r, sigma, option_type, q, include_second_order, seed=None):
        vals, _ = _hip.jd_greeks_fd(S, K, T, r, sigma, q, option_type == "call", self.jd._jd(), self.n_paths, self.n_steps, self.seed,
                                    self.antithetic, include_second_order, want_evals=False)
        keys = ("price", "delta", "gamma", "vega", "theta", "rho", "vanna", "charm", "vomma")
        return OrderedDict((k, np.float64(v)) for k, v in zip(keys if include_second_order else keys[:6], vals))


def greeks_jump_monte_carlo(model, S: float, K: float, T: float, r: float, sigma: float, option_type: str = "call", q: float = 0.0,
                            include_second_order: bool = True, **adapter_kwargs):
    """compute_greeks_unified over JumpMCAdapter(model, **adapter_kwargs): the finite-difference Greeks of the Monte Carlo price in one
    launch."""
    from .greeks import compute_greeks_unified

    return compute_greeks_unified(JumpMCAdapter(model, **adapter_kwargs), S, K, T, r, sigma, option_type, q, include_second_order)
