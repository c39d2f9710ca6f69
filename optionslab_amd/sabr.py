"""SABRModel on the device path engine (reference: src/pricing_models/sabr.py).

The reference's SABR is Hagan's implied-volatility expansion behind Black's formula, and a calibration of (alpha, rho, nu) to a smile.
Both are restated here in this package's own code and tied to the reference by tests/golden/sabr.json: `implied_vol`, `smile`, `price`,
`_black_price`, `calibrate_sabr` with the reference's start, bounds (alpha capped at 2.0 included), L-BFGS-B and 200 iterations.

Additive: Monte Carlo paths of the process itself (include/olmc_sabr.h) -- dF = sigma F^beta dW1, dsigma = nu sigma dW2, absorbed at 0
for beta < 1 -- where the expansion degrades (large nu, rho towards -1, the wings) and for the payoffs it does not cover: Europeans,
Asians, barriers, lookbacks and a strike x maturity surface, each in one launch, and the Monte Carlo smile.  The methods take the
forward F where DupireLocalVol's take S, and no q.  `SABRModelQMC` (`model.qmc()`) runs the same methods on scrambled-Sobol points
(include/olmc_sabr_qmc.h).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Literal, Optional, Tuple

import numpy as np

from . import _hip
from ._paths import _asian_payoff, _barrier_kind, _check_barrier, _check_sizes, _fill_surface, _lookback_payoff, _result, _seed, _strike_list, _surface_steps
from .black_scholes import implied_volatility

_ATM_WIDTH = 1e-10           # |K - F| below this is at the money (sabr.py:91)
_SMALL_Z = 1e-7              # |z| below this: z / x(z) is 1 (sabr.py:105)
_N_PATHS, _N_STEPS = 100_000, 252          # DupireLocalVol's defaults
_CELLS = 16                  # strikes of one smile launch (OLMC_MAX_BATCH)


def _ndtr(x):
    from scipy.special import ndtr

    return ndtr(x)


@dataclass
class SABRModel:
    """alpha: the initial volatility sigma_0; beta: the CEV exponent (0 normal, 1 lognormal); rho: the correlation of forward and
    volatility; nu: the volatility of volatility.  Field names, order and refusals are the reference's."""

    alpha: float
    beta: float
    rho: float
    nu: float

    def __post_init__(self):
        if self.alpha <= 0:
            raise ValueError("alpha must be positive")
        if not 0 <= self.beta <= 1:
            raise ValueError("beta must be in [0, 1]")
        if not -1 <= self.rho <= 1:
            raise ValueError("rho must be in [-1, 1]")
        if self.nu < 0:
            raise ValueError("nu must be non-negative")

    # ------------------------------------------------------------------ Hagan's expansion ----
    def _time_correction(self, scale: float, T: float) -> float:
        """1 + (the three first-order terms) T, with scale = (F K)^((1 - beta) / 2), or F^(1 - beta) at the money."""
        gap = 1 - self.beta
        cev = gap**2 / 24 * self.alpha**2 / scale**2
        cross = 0.25 * self.rho * self.beta * self.nu * self.alpha / scale
        vol_of_vol = (2 - 3 * self.rho**2) * self.nu**2 / 24
        return 1 + (cev + cross + vol_of_vol) * T

    def implied_vol(self, F: float, K: float, T: float) -> float:
        """The lognormal implied volatility of Hagan et al. (2002).  T <= 0 answers alpha; |K - F| < 1e-10 the at-the-money form."""
        if T <= 0:
            return self.alpha
        if abs(K - F) < _ATM_WIDTH:
            return self._atm_vol(F, T)
        gap = 1 - self.beta
        moneyness = np.log(F / K)
        scale = (F * K) ** (gap / 2)
        z = self.nu / self.alpha * scale * moneyness
        x_of_z = np.log((np.sqrt(1 - 2 * self.rho * z + z**2) + z - self.rho) / (1 - self.rho))
        stretch = 1.0 if abs(z) < _SMALL_Z else z / x_of_z
        level = self.alpha / (scale * (1 + gap**2 / 24 * moneyness**2 + gap**4 / 1920 * moneyness**4))
        return level * stretch * self._time_correction(scale, T)

    def _atm_vol(self, F: float, T: float) -> float:
        scale = F ** (1 - self.beta)
        return self.alpha / scale * self._time_correction(scale, T)

    def smile(self, F: float, T: float, strikes: np.ndarray) -> np.ndarray:
        return np.array([self.implied_vol(F, K, T) for K in strikes])

    def price(self, F: float, K: float, T: float, r: float, option_type: Literal["call", "put"] = "call") -> float:
        """Black's formula at implied_vol(F, K, T), discounted at r."""
        return self._black_price(F, K, T, r, self.implied_vol(F, K, T), option_type)

    @staticmethod
    def _black_price(F: float, K: float, T: float, r: float, sigma: float, option_type: str) -> float:
        """Black (1976) on the forward.  T <= 0 pays the intrinsic value; anything but "call" prices as a put."""
        discount = np.exp(-r * T)
        call = option_type == "call"
        if T <= 0:
            return discount * (max(F - K, 0) if call else max(K - F, 0))
        total = sigma * np.sqrt(T)
        d_plus = (np.log(F / K) + 0.5 * sigma**2 * T) / total
        d_minus = d_plus - total
        if call:
            return discount * (F * _ndtr(d_plus) - K * _ndtr(d_minus))
        return discount * (K * _ndtr(-d_minus) - F * _ndtr(-d_plus))

    # ------------------------------------------------------------------ Monte Carlo on the device ----
    def _model(self):
        return (self.alpha, self.beta, self.rho, self.nu)

    @staticmethod
    def _sizes(F, n_paths, n_steps, seed, default_paths=_N_PATHS):
        if not F > 0:
            raise ValueError("F must be positive")
        n_paths = default_paths if n_paths is None else n_paths
        n_steps = _N_STEPS if n_steps is None else n_steps
        _check_sizes(n_paths, n_steps)
        return n_paths, n_steps, _seed(seed)

    # The three device calls, each on the sizes and seed _sizes settled: what SABRModelQMC overrides.
    def _device_price(self, F, K, T, r, is_call, payoff, barrier, n_paths, n_steps, seed, antithetic):
        return _hip.sabr_price(F, K, T, r, is_call, self._model(), payoff, barrier, n_paths, n_steps, seed, antithetic)

    def _device_paths(self, F, T, n_paths, n_steps, seed, mirror):
        return _hip.sabr_paths(F, T, self._model(), n_paths, n_steps, seed, mirror=mirror, path_major=True)

    def _device_surface(self, F, T, r, is_call, strikes, steps, n_paths, n_steps, seed, antithetic):
        return _hip.sabr_surface_prices(F, T, r, is_call, self._model(), strikes, steps, n_paths, n_steps, seed, antithetic)

    def _price_payoff(self, payoff, barrier, F, K, T, r, option_type, n_paths, n_steps, seed, antithetic, return_error):
        n_paths, n_steps, s = self._sizes(F, n_paths, n_steps, seed)
        return _result(self._device_price(F, K, T, r, option_type == "call", payoff, barrier, n_paths, n_steps, s, antithetic), return_error)

    def price_monte_carlo(self, F: float, K: float, T: float, r: float, option_type: Literal["call", "put"] = "call",
                          n_paths: Optional[int] = None, n_steps: Optional[int] = None, seed: Optional[int] = None, antithetic: bool = False,
                          return_error: bool = False):
        """exp(-r T) mean(max(+-(F_n - K), 0)) over paths of include/olmc_sabr.h's recursion: one launch that stores no path.  The
        paths are simulate_paths' rows for the same seed.  n_paths, n_steps: None takes 100000 and 252; seed=None draws one.  antithetic
        also walks the mirrored path (-Z1, -Z2'), under its own volatility (2 n_paths samples).  Anything but "call" prices as a put."""
        return self._price_payoff(_hip.SABR_EUROPEAN, 0.0, F, K, T, r, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def simulate_paths(self, F: float, T: float, n_paths: int = 1000, n_steps: int = 252, seed: Optional[int] = None,
                       mirror: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """The forward and volatility matrices, each (n_paths, n_steps + 1), of price_monte_carlo's recursion for the same seed; column
        0 is (F, alpha) as given.  mirror=True gives the antithetic leg."""
        n_paths, n_steps, s = self._sizes(F, n_paths, n_steps, seed)
        return self._device_paths(F, T, n_paths, n_steps, s, mirror)

    def price_asian(self, F: float, K: float, T: float, r: float, option_type: Literal["call", "put"] = "call",
                    avg_type: Literal["arithmetic", "geometric"] = "arithmetic", n_paths: Optional[int] = None, n_steps: Optional[int] = None,
                    seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False):
        """max(+-(A - K), 0), A the arithmetic or geometric mean of simulate_paths' forward over dates 1 .. n_steps.  An absorbed path
        has a geometric mean of 0."""
        return self._price_payoff(_asian_payoff(avg_type), 0.0, F, K, T, r, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_barrier(self, F: float, K: float, T: float, r: float, barrier: float, option_type: Literal["call", "put"] = "call",
                      barrier_type: Literal["up-and-out", "up-and-in", "down-and-out", "down-and-in"] = "up-and-out",
                      n_paths: Optional[int] = None, n_steps: Optional[int] = None, seed: Optional[int] = None, antithetic: bool = False,
                      return_error: bool = False):
        """The barrier option monitored at dates 0 .. n_steps of simulate_paths' forward, with HestonPricer.price_barrier's reading of
        barrier_type and its date-0 decision.  An absorbed path has hit every down barrier.  Refused: barrier <= 0."""
        _check_barrier(barrier)
        return self._price_payoff(_barrier_kind(barrier_type), barrier, F, K, T, r, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_lookback(self, F: float, K: float, T: float, r: float, option_type: Literal["call", "put"] = "call",
                       lookback_type: Literal["floating", "fixed"] = "floating", n_paths: Optional[int] = None, n_steps: Optional[int] = None,
                       seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False):
        """The lookback option on the extrema of simulate_paths' forward over dates 0 .. n_steps."""
        return self._price_payoff(_lookback_payoff(lookback_type), 0.0, F, K, T, r, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_surface(self, F: float, strikes, maturities, r: float, option_type: Literal["call", "put"] = "call",
                      n_paths: Optional[int] = None, n_steps: Optional[int] = None, seed: Optional[int] = None, antithetic: bool = False,
                      return_error: bool = False):
        """European prices on a strike x maturity grid from ONE set of paths: an array (len(strikes), len(maturities)), with return_error
        (prices, std_errors).  The grid, its refusals and the launches of at most 16 cells are HestonPricer.price_surface's."""
        ks = _strike_list(strikes)
        n_paths, n_steps, s = self._sizes(F, n_paths, n_steps, seed)
        T, steps = _surface_steps(maturities, n_steps)
        return _fill_surface(ks, steps, lambda cell_k, cell_m: self._device_surface(F, T, r, option_type == "call", cell_k, cell_m, n_paths, n_steps, s,
                                                                                   antithetic), return_error)

    def smile_monte_carlo(self, F: float, T: float, strikes, n_paths: Optional[int] = None, n_steps: Optional[int] = None,
                          seed: Optional[int] = None, antithetic: bool = False) -> np.ndarray:
        """The Black implied volatility of the Monte Carlo price at every strike: out-of-the-money options (puts below F, calls from F
        up) at r = 0 on one seed, at most two launches per 16 strikes, each price inverted by implied_volatility(S = F, r = q = 0).
        NaN where a price lies outside the no-arbitrage bounds (a wing no path reached)."""
        ks = _strike_list(strikes)
        n_paths, n_steps, s = self._sizes(F, n_paths, n_steps, seed)
        vols = np.full(len(ks), np.nan)
        for a in range(0, len(ks), _CELLS):
            chunk = range(a, min(a + _CELLS, len(ks)))
            for is_call in (False, True):
                idx = [i for i in chunk if (ks[i] >= F) == is_call]
                if not idx:
                    continue
                sts = self._device_surface(F, T, 0.0, is_call, [ks[i] for i in idx], [n_steps] * len(idx), n_paths, n_steps, s, antithetic)
                for i, st in zip(idx, sts):
                    try:
                        vols[i] = implied_volatility(st.price, F, ks[i], T, 0.0, "call" if is_call else "put", 0.0)
                    except ValueError:
                        pass
        return vols

    def qmc(self, path_construction: Literal["bridge", "sequential"] = "bridge") -> "SABRModelQMC":
        """This model on scrambled-Sobol points: a view with the same four parameters."""
        return SABRModelQMC(self.alpha, self.beta, self.rho, self.nu, path_construction=path_construction)


@dataclass
class SABRModelQMC(SABRModel):
    """SABRModel on scrambled-Sobol paths (include/olmc_sabr_qmc.h): every Monte Carlo method keeps its signature and meaning,
    simulate_paths(mirror=), price_surface, smile_monte_carlo and antithetic included; n_paths counts Sobol points and path i is point i
    of scipy.stats.qmc.Sobol(d = 2 n_steps, scramble=True, seed), two dimensions per step.  path_construction="bridge" (the default, at
    most 1024 steps) builds the two Brownian paths by the breadth-first bridge and steps on their increments, "sequential" gives step t
    dimensions 2t and 2t + 1 (at most 10600 steps).  The table refusals are heston._qmc_tables', ValueErrors raised before the device is
    touched.  return_error's figure is the naive standard error of the payoffs: for Sobol points it overstates the error.  With
    seed=None every call draws a scramble of its own; SABRMCAdapter(model.qmc(), ...) differentiates on the same points at its fixed
    seed, one launch per bump."""

    path_construction: str = "bridge"

    def __post_init__(self):
        super().__post_init__()
        if self.path_construction not in ("bridge", "sequential"):
            raise ValueError("path_construction must be 'bridge' or 'sequential'")

    def _sobol(self, n_paths, n_steps, seed):
        """(sv, shift, bridge) of Sobol(d = 2 n_steps, seed); sobol_tables caches them, so price_surface's launches share one pair."""
        from .heston import _qmc_tables

        return _qmc_tables("qmc", self.path_construction, n_paths, n_steps, seed)

    def _device_price(self, F, K, T, r, is_call, payoff, barrier, n_paths, n_steps, seed, antithetic):
        sv, shift, bridge = self._sobol(n_paths, n_steps, seed)
        return _hip.sabrq_price(F, K, T, r, is_call, self._model(), payoff, barrier, n_paths, sv, shift, bridge, antithetic)

    def _device_paths(self, F, T, n_paths, n_steps, seed, mirror):
        sv, shift, bridge = self._sobol(n_paths, n_steps, seed)
        return _hip.sabrq_paths(F, T, self._model(), n_paths, sv, shift, bridge, mirror=mirror, path_major=True)

    def _device_surface(self, F, T, r, is_call, strikes, steps, n_paths, n_steps, seed, antithetic):
        sv, shift, bridge = self._sobol(n_paths, n_steps, seed)
        return _hip.sabrq_surface_prices(F, T, r, is_call, self._model(), strikes, steps, n_paths, sv, shift, bridge, antithetic)


def calibrate_sabr(F: float, T: float, strikes: np.ndarray, market_vols: np.ndarray, beta: float = 0.5,
                   initial_guess: Optional[dict] = None) -> SABRModel:
    """(alpha, rho, nu) at fixed beta by least squares on the smile, with the reference's rules: the start is the market volatility of the
    strike nearest F times F^(1 - beta), rho = -0.3, nu = 0.4; L-BFGS-B within alpha in [0.001, 2.0], rho in [-0.99, 0.99], nu in
    [0.001, 2.0], at most 200 iterations; a point outside the model's domain, or one whose smile cannot be evaluated, costs 1e10."""
    from scipy.optimize import minimize

    if initial_guess is None:
        nearest = np.argmin(np.abs(strikes - F))
        initial_guess = {"alpha": market_vols[nearest] * F ** (1 - beta), "rho": -0.3, "nu": 0.4}

    def misfit(x):
        alpha, rho, nu = x
        if alpha <= 0 or nu < 0 or not -0.99 <= rho <= 0.99:
            return 1e10
        try:
            return np.sum((SABRModel(alpha, beta, rho, nu).smile(F, T, strikes) - market_vols) ** 2)
        except Exception:
            return 1e10

    fit = minimize(misfit, [initial_guess[name] for name in ("alpha", "rho", "nu")], method="L-BFGS-B",
                   bounds=[(0.001, 2.0), (-0.99, 0.99), (0.001, 2.0)], options={"maxiter": 200})
    alpha, rho, nu = fit.x
    return SABRModel(alpha, beta, rho, nu)


# ------------------------------------------------------------------ Greeks ----
class SABRAdapter:
    """PricerProtocol over SABRModel (unified_greeks.py:107-129): the forward is S e^{(r - q) T}, the price Hagan's; sigma is ignored."""

    def __init__(self, sabr_model):
        self.sabr = sabr_model

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kwargs) -> float:
        return self.sabr.price(S * np.exp((r - q) * T), K, T, r, option_type)


class SABRMCAdapter:
    """The same over price_monte_carlo at a fixed seed: every bump of compute_greeks_unified walks the same draws (common random
    numbers), one launch per evaluation."""

    def __init__(self, sabr_model, n_paths: int = _N_PATHS, n_steps: int = _N_STEPS, seed: int = 0, antithetic: bool = False):
        self.sabr = sabr_model
        self.n_paths, self.n_steps, self.seed, self.antithetic = n_paths, n_steps, seed, antithetic

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kwargs) -> float:
        return float(self.sabr.price_monte_carlo(S * np.exp((r - q) * T), K, T, r, option_type, self.n_paths, self.n_steps, self.seed, self.antithetic))


def greeks_sabr(sabr_model, S: float, K: float, T: float, r: float, option_type: str = "call", q: float = 0.0) -> "OrderedDict[str, float]":
    """compute_greeks_unified over SABRAdapter, with the reference's placeholder sigma of 0.2 (ignored by the model)."""
    from .greeks import compute_greeks_unified

    return compute_greeks_unified(SABRAdapter(sabr_model), S, K, T, r, 0.2, option_type, q)
