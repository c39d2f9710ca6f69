"""HestonPricer on the device step loop (reference: src/pricing_models/heston.py:41-305).

`price_monte_carlo` (full-truncation Euler, :184-255) runs on the GPU: two normals per step,
(ln S, v) in fp64 registers.  `price_european` (:131-182) is the reference's semi-analytic
Lewis/Gatheral quadrature -- scalar host arithmetic, kept so `HestonAdapter`-style callers and
accuracy checks have the same oracle the reference has; it is not a Monte Carlo path.

Additive: ``method="qmc"`` runs `price_monte_carlo` and `simulate_paths` on scrambled-Sobol points, two dimensions per step
(_qmc_tables below, include/olmc.h "quasi-Monte Carlo Heston"), by default with two Brownian bridges.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Tuple, Literal, Optional

import numpy as np

from . import _hip


def _qmc_tables(method: str, path_construction: str, n_paths: int, n_steps: int, seed: Optional[int]):
    """exotic._qmc_tables with two Sobol dimensions per step: tables of Sobol(d=2 n_steps), at most 10600 steps."""
    from .exotic import _qmc_tables as tables

    return tables(method, path_construction, n_paths, n_steps, seed, dims_per_step=2)


@dataclass
class HestonPricer:
    kappa: float
    theta: float
    sigma_v: float
    rho: float
    v0: float

    def __post_init__(self):     # heston.py:61-78
        if self.kappa <= 0:
            raise ValueError("kappa must be positive")
        if self.theta <= 0:
            raise ValueError("theta must be positive")
        if self.sigma_v <= 0:
            raise ValueError("sigma_v must be positive")
        if not -1 <= self.rho <= 1:
            raise ValueError("rho must be in [-1, 1]")
        if self.v0 <= 0:
            raise ValueError("v0 must be positive")
        feller = 2 * self.kappa * self.theta - self.sigma_v**2
        if feller < 0:
            warnings.warn(f"Feller condition not satisfied (2κθ - σᵥ² = {feller:.4f} < 0). "
                          "Variance may hit zero in simulations.")

    def _characteristic_function(self, u, S, K, T, r, q):       # :80-129
        kappa, theta, sigma_v, rho, v0 = self.kappa, self.theta, self.sigma_v, self.rho, self.v0
        x = np.log(S / K) + (r - q) * T
        alpha = -0.5 * u * (u + 1j)
        beta = kappa - rho * sigma_v * 1j * u
        d = np.sqrt(beta**2 - 4 * alpha * (0.5 * sigma_v**2))
        r_minus = (beta - d) / (sigma_v**2)
        g = r_minus / ((beta + d) / (sigma_v**2))
        e = np.exp(-d * T)
        big_c = kappa * (r_minus * T - (2 / sigma_v**2) * np.log((1 - g * e) / (1 - g)))
        big_d = r_minus * (1 - e) / (1 - g * e)
        return np.exp(big_c * theta + big_d * v0 + 1j * u * x)

    def price_european(self, S: float, K: float, T: float, r: float, q: float = 0.0,
                       option_type: Literal["call", "put"] = "call") -> float:
        from scipy.integrate import quad

        if T <= 0:
            return max(S - K, 0) if option_type == "call" else max(K - S, 0)
        fwd = S * np.exp((r - q) * T)

        def integrand(u):
            cf = self._characteristic_function(u - 0.5j, S, K, T, r, q)
            return np.real(np.exp(-1j * u * np.log(K / fwd)) * cf / (u**2 + 0.25))

        integral, _ = quad(integrand, 0, 100, limit=100)
        call = S * np.exp(-q * T) - (np.sqrt(K * fwd) / np.pi) * np.exp(-r * T) * integral
        if option_type == "call":
            return max(call, 0.0)
        return max(call - S * np.exp(-q * T) + K * np.exp(-r * T), 0.0)

    def price_monte_carlo(self, S: float, K: float, T: float, r: float, q: float = 0.0,
                          option_type: Literal["call", "put"] = "call", n_paths: int = 100000, n_steps: int = 252,
                          seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                          method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """method (additive): "pseudo" (default) = the Philox paths; "qmc" = scrambled-Sobol paths: `seed` is the scramble seed of
        scipy.stats.qmc.Sobol(d=2 n_steps, scramble=True, seed=seed) (None draws one), point k drives path k through
        z = norm.ppf(clip(u, 1e-10, 1 - 1e-10)); n_paths <= 2**30, n_steps <= 10600.
        path_construction (read only with method="qmc"): "bridge" (default) = two Brownian bridges in breadth-first order, W1 on the
        even and W2 on the odd dimensions (dimensions 0 and 1 set the two terminal values: include/olmc.h), step t taking their
        increments as Z1 and Z2', at most 1024 steps; "sequential" = dimensions 2t, 2t + 1 are Z1, Z2' of step t.
        With method="qmc", antithetic=True also prices the mirrored point -z (2 n_paths samples), and return_error's standard error is
        the naive per-path one: for Sobol points it is not a confidence interval (it overstates the error).
        Refused (ValueError, before the device is touched): an unknown method or path_construction, and with method="qmc"
        n_steps > 10600, n_steps > 1024 with the bridge, n_paths > 2**30."""
        if n_paths < 1 or n_steps < 1:
            raise ValueError("n_paths and n_steps must be >= 1")
        qmc = _qmc_tables(method, path_construction, n_paths, n_steps, seed)
        if qmc is not None:
            sv, shift, bridge = qmc
            st = _hip.heston_qmc(S, K, T, r, q, option_type == "call", self.kappa, self.theta, self.sigma_v, self.rho, self.v0, n_paths,
                                 sv, shift, bridge, antithetic)
            return (np.float64(st.price), float(st.std_error)) if return_error else np.float64(st.price)
        s = seed if seed is not None else int(np.random.default_rng().integers(0, 2**31))
        st = _hip.heston(S, K, T, r, q, option_type == "call", self.kappa, self.theta, self.sigma_v, self.rho, self.v0,
                         n_paths, n_steps, s, antithetic)
        return (np.float64(st.price), float(st.std_error)) if return_error else np.float64(st.price)


    def simulate_paths(self, S: float, T: float, r: float, q: float = 0.0, n_paths: int = 1000, n_steps: int = 252,
                       seed: Optional[int] = None, *, method: Literal["pseudo", "qmc"] = "pseudo",
                       path_construction: Literal["bridge", "sequential"] = "bridge") -> Tuple[np.ndarray, np.ndarray]:
        """heston.py:257-305: (spot_paths, variance_paths), each (n_paths, n_steps + 1), column 0 = (S, v0).
        The states of price_monte_carlo's recursion for the same seed, method and path_construction (additive, as there)."""
        if n_paths < 1 or n_steps < 1:
            raise ValueError("n_paths and n_steps must be >= 1")
        qmc = _qmc_tables(method, path_construction, n_paths, n_steps, seed)
        if qmc is not None:
            sv, shift, bridge = qmc
            return _hip.heston_qmc_paths(S, T, r, q, self.kappa, self.theta, self.sigma_v, self.rho, self.v0, n_paths, sv, shift, bridge,
                                         path_major=True)
        s = seed if seed is not None else int(np.random.default_rng().integers(0, 2**31))
        return _hip.heston_paths(S, T, r, q, self.kappa, self.theta, self.sigma_v, self.rho, self.v0, n_paths, n_steps, s, path_major=True)

    def _price_path_payoff(self, payoff: int, barrier: float, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error,
                           method, path_construction):
        """One launch of the path-payoff kernels (include/olmc.h "path payoffs under Heston") under price_monte_carlo's conventions."""
        if n_paths < 1 or n_steps < 1:
            raise ValueError("n_paths and n_steps must be >= 1")
        model = (self.kappa, self.theta, self.sigma_v, self.rho, self.v0)
        qmc = _qmc_tables(method, path_construction, n_paths, n_steps, seed)
        if qmc is not None:
            sv, shift, bridge = qmc
            st = _hip.heston_qmc_path_payoff(S, K, T, r, q, option_type == "call", *model, payoff, barrier, n_paths, sv, shift, bridge, antithetic)
        else:
            s = seed if seed is not None else int(np.random.default_rng().integers(0, 2**31))
            st = _hip.heston_path_payoff(S, K, T, r, q, option_type == "call", *model, payoff, barrier, n_paths, n_steps, s, antithetic)
        return (np.float64(st.price), float(st.std_error)) if return_error else np.float64(st.price)

    def price_asian(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                    avg_type: Literal["arithmetic", "geometric"] = "arithmetic", n_paths: int = 100000, n_steps: int = 252,
                    seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                    method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """The Asian option max(+-(A - K), 0) under this model, A the arithmetic or geometric mean of the spot over dates 1 .. n_steps: what
        AsianOption.price (exotic_options.py:97-131) computes from simulate_paths' spot matrix for the same seed, method and
        path_construction, in one launch that stores no path.  seed, antithetic, return_error, method and path_construction as
        price_monte_carlo: with method="qmc" the standard error is the naive per-path one, not a confidence interval (it overstates the
        error).  Refused (ValueError, before the device is touched): an unknown avg_type, and what price_monte_carlo refuses."""
        if avg_type not in ("arithmetic", "geometric"):
            raise ValueError("avg_type must be 'arithmetic' or 'geometric'")
        payoff = _hip.PATH_ASIAN_GEOMETRIC if avg_type == "geometric" else _hip.PATH_ASIAN_ARITHMETIC
        return self._price_path_payoff(payoff, 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error, method,
                                       path_construction)

    def price_barrier(self, S: float, K: float, T: float, r: float, barrier: float, q: float = 0.0,
                      option_type: Literal["call", "put"] = "call",
                      barrier_type: Literal["up-and-out", "up-and-in", "down-and-out", "down-and-in"] = "up-and-out", n_paths: int = 100000,
                      n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                      method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """The barrier option under this model: max(+-(S_n - K), 0) where the barrier, monitored at dates 0 .. n_steps of simulate_paths' spot
        matrix (date 0 is S itself: S >= barrier for an up barrier, S <= barrier for a down one), leaves it active -- what
        BarrierOption.price (exotic_options.py:174-224) computes from that matrix, in one launch that stores no path.  barrier_type is read
        as the reference's class reads it: startswith("up") and endswith("out").  After date 0 the kernel decides in log space, ln(S_t / S)
        against ln(barrier / S), where the matrix route compares exp(ln S_t) with the barrier: the two agree except for a path within
        rounding (about 1e-16 relative) of the level, which can decide differently.  The rest as price_asian; also refused: barrier <= 0."""
        if barrier <= 0:
            raise ValueError("Barrier must be positive")
        kind = ("up" if barrier_type.startswith("up") else "down") + ("-and-out" if barrier_type.endswith("out") else "-and-in")
        return self._price_path_payoff(_hip.BARRIER_KINDS[kind], barrier, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic,
                                       return_error, method, path_construction)

    def price_lookback(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                       lookback_type: Literal["floating", "fixed"] = "floating", n_paths: int = 100000, n_steps: int = 252,
                       seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                       method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """The lookback option under this model on the extrema of simulate_paths' spot matrix over dates 0 .. n_steps: floating call S_n -
        S_min, floating put S_max - S_n, fixed call max(S_max - K, 0), fixed put max(K - S_min, 0) (LookbackOption.price,
        exotic_options.py:347-401), in one launch that stores no path.  The rest as price_asian; also refused: an unknown lookback_type."""
        if lookback_type not in ("floating", "fixed"):
            raise ValueError("lookback_type must be 'floating' or 'fixed'")
        payoff = _hip.LOOKBACK_FIXED if lookback_type == "fixed" else _hip.LOOKBACK_FLOATING
        return self._price_path_payoff(payoff, 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error, method,
                                       path_construction)


class HestonAdapter:
    """unified_greeks.py:74-104: sigma -> v0 = sigma^2, prices with the semi-analytic formula."""

    def __init__(self, heston_pricer):
        self.heston = heston_pricer
        self._original_v0 = heston_pricer.v0

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kwargs) -> float:
        self.heston.v0 = sigma**2
        try:
            return self.heston.price_european(S, K, T, r, q, option_type)
        finally:
            self.heston.v0 = self._original_v0


def greeks_heston(heston_pricer, S: float, K: float, T: float, r: float, sigma: float, option_type: str = "call", q: float = 0.0):
    """unified_greeks.py:375-388"""
    from .greeks import compute_greeks_unified

    return compute_greeks_unified(HestonAdapter(heston_pricer), S, K, T, r, sigma, option_type, q)
