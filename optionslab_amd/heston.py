"""HestonPricer on the device step loop (reference: src/pricing_models/heston.py:41-305).

`price_monte_carlo` (full-truncation Euler, :184-255) runs on the GPU: two normals per step,
(ln S, v) in fp64 registers.  `price_european` (:131-182) is the reference's semi-analytic
Lewis/Gatheral quadrature -- scalar host arithmetic, kept so `HestonAdapter`-style callers and
accuracy checks have the same oracle the reference has; it is not a Monte Carlo path.

Additive: ``method="qmc"`` runs `price_monte_carlo` and `simulate_paths` on scrambled-Sobol points, two dimensions per step
(_qmc_tables below, include/olmc.h "quasi-Monte Carlo Heston"), by default with two Brownian bridges.
Additive: ``scheme="qe"`` (keyword-only; "euler" is the default and today's code path) discretises with Andersen's quadratic-exponential
scheme (include/olmc.h "Heston, quadratic-exponential scheme") in `price_monte_carlo`, `simulate_paths`, `price_surface`,
`calibration_objective` and `calibrate_heston`; the path payoffs (`price_asian`, `price_barrier`, `price_lookback`) stay on Euler.
Additive: `price_american` prices the American option by least-squares Monte Carlo on `simulate_paths`' matrices, regressing on the
state (S_t, v_t) (include/olha.h), with either scheme and either method.
"""
from __future__ import annotations

import copy
import struct
import warnings
from collections import OrderedDict
from dataclasses import dataclass
from typing import Tuple, Literal, Optional

import numpy as np

from . import _hip
from ._paths import _SURFACE_CELLS, _asian_payoff, _barrier_kind, _check_barrier, _check_sizes, _fill_surface, _lookback_payoff, _result, _seed, _strike_list
from ._paths import _grid_steps, _surface_launches, _surface_steps      # noqa: F401 -- the surface grid moved there; its names stay importable from here

_SCENARIO_KEYS = ("kappa", "theta", "sigma_v", "rho", "v0")
_STEPS_PER_YEAR = {"euler": 64, "qe": 16}      # calibrate_heston's grid when n_steps is None


def _qmc_tables(method: str, path_construction: str, n_paths: int, n_steps: int, seed: Optional[int]):
    """exotic._qmc_tables with two Sobol dimensions per step: tables of Sobol(d=2 n_steps), at most 10600 steps."""
    from .exotic import _qmc_tables as tables

    return tables(method, path_construction, n_paths, n_steps, seed, dims_per_step=2)


def _draws(method: str, path_construction: str, n_paths: int, n_steps: int, seed: Optional[int]):
    """exotic._draws with two Sobol dimensions per step: on Sobol points (True, (n_paths, sv, shift, bridge)), else (False, (n_paths,
    n_steps, seed)) -- what every Heston binding takes between its contract and its antithetic or layout flag."""
    from .exotic import _draws as draws

    return draws(method, path_construction, n_paths, n_steps, seed, dims_per_step=2)


# what -> _hip's wrapper by (qe, sobol): Euler or QE, on Philox draws or Sobol points.  The scenario kernels, the path payoffs and the
# plain price have no QE form (scheme="qe" prices through the one-cell surface).
_BINDINGS = {
    "price": {(False, False): "heston", (False, True): "heston_qmc"},
    "path_payoff": {(False, False): "heston_path_payoff", (False, True): "heston_qmc_path_payoff"},
    "scenarios": {(False, False): "heston_scenarios", (False, True): "heston_qmc_scenarios"},
    "surface": {(False, False): "heston_surface", (False, True): "heston_qmc_surface",
                (True, False): "heston_qe_surface", (True, True): "heston_qe_qmc_surface"},
    "paths": {(False, False): "heston_paths", (False, True): "heston_qmc_paths",
              (True, False): "heston_qe_paths", (True, True): "heston_qe_qmc_paths"},
}


def _binding(what: str, sobol: bool, qe: bool = False):
    """The four-way choice, written once (looked up in _hip at the call, as a plain _hip.name would be)."""
    return getattr(_hip, _BINDINGS[what][qe, sobol])


def _check_scheme(scheme: str, method: str, path_construction: str) -> bool:
    """True for scheme="qe"; ValueError (before the device is touched) for an unknown scheme and for QE on bridged Sobol points."""
    if scheme not in ("euler", "qe"):
        raise ValueError("scheme must be 'euler' or 'qe'")
    if scheme == "qe" and method == "qmc" and path_construction == "bridge":
        raise ValueError("scheme='qe' with method='qmc' takes path_construction='sequential': pass path_construction='sequential' "
                         "(QE's variance draw is a uniform, not a Brownian increment, so there is nothing for a bridge to build)")
    return scheme == "qe"


def _check_euler_only(scheme: str, what: str) -> None:
    if scheme not in ("euler", "qe"):
        raise ValueError("scheme must be 'euler' or 'qe'")
    if scheme == "qe":
        raise ValueError(f"{what} runs the Euler scheme only: the fused scenario kernels have no quadratic-exponential form yet")


def _recursion_key(T, kappa, theta, sigma_v, rho, v0) -> bytes:
    """What two scenarios must share to share a recursion: the six doubles, compared bit for bit (0.04 and 0.2**2 differ)."""
    return struct.pack("<6d", T, kappa, theta, sigma_v, rho, v0)


def _scenario_launches(keys, max_scenarios: int = _SURFACE_CELLS, max_recursions: int = _hip.HESTON_MAX_RECURSIONS):
    """A list of scenarios, given by their recursion keys, cut greedily and in the caller's order into launches of at most 16 scenarios
    and at most 6 distinct recursions: lists of indices, every index once.  A launch ends where the next scenario would be its 17th or
    would bring a seventh recursion."""
    launches, current, seen = [], [], set()
    for i, key in enumerate(keys):
        if current and (len(current) == max_scenarios or (key not in seen and len(seen) == max_recursions)):
            launches.append(current)
            current, seen = [], set()
        current.append(i)
        seen.add(key)
    if current:
        launches.append(current)
    return launches


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

    def _model(self):
        return self.kappa, self.theta, self.sigma_v, self.rho, self.v0

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
                          method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge",
                          scheme: Literal["euler", "qe"] = "euler"):
        """method (additive): "pseudo" (default) = the Philox paths; "qmc" = scrambled-Sobol paths: `seed` is the scramble seed of
        scipy.stats.qmc.Sobol(d=2 n_steps, scramble=True, seed=seed) (None draws one), point k drives path k through
        z = norm.ppf(clip(u, 1e-10, 1 - 1e-10)); n_paths <= 2**30, n_steps <= 10600.
        path_construction (read only with method="qmc"): "bridge" (default) = two Brownian bridges in breadth-first order, W1 on the
        even and W2 on the odd dimensions (dimensions 0 and 1 set the two terminal values: include/olmc.h), step t taking their
        increments as Z1 and Z2', at most 1024 steps; "sequential" = dimensions 2t, 2t + 1 are Z1, Z2' of step t.
        With method="qmc", antithetic=True also prices the mirrored point -z (2 n_paths samples), and return_error's standard error is
        the naive per-path one: for Sobol points it is not a confidence interval (it overstates the error).
        Refused (ValueError, before the device is touched): an unknown method or path_construction, and with method="qmc"
        n_steps > 10600, n_steps > 1024 with the bridge, n_paths > 2**30.
        scheme (additive): "euler" (default) = the reference's full-truncation Euler step; "qe" = Andersen's quadratic-exponential
        scheme (include/olmc.h "Heston, quadratic-exponential scheme"), priced as the one-cell surface (K, T) of price_surface(...,
        scheme="qe") -- the same bits.  QE samples the variance from a distribution matched to its exact conditional mean and variance
        and needs 4-16 steps per year where Euler needs hundreds when the Feller condition fails; its Philox stream (one block per
        step, its own tag) and its Sobol draws (dimension 2t = the variance's uniform, 2t + 1 = the spot's normal) are not Euler's, so
        equal seeds give other paths.  With method="qmc" it takes path_construction="sequential" only: the default "bridge" is refused
        (ValueError, before the device is touched), as is an unknown scheme."""
        _check_sizes(n_paths, n_steps)
        if _check_scheme(scheme, method, path_construction):
            prices, errors = self.price_surface(S, [K], [T], r, q, option_type, n_paths, n_steps, seed, antithetic, return_error=True,
                                                method=method, path_construction=path_construction, scheme="qe")
            return (np.float64(prices[0, 0]), float(errors[0, 0])) if return_error else np.float64(prices[0, 0])
        sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        return _result(_binding("price", sobol)(S, K, T, r, q, option_type == "call", *self._model(), *run, antithetic), return_error)

    def price_surface(self, S: float, strikes, maturities, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                      n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False,
                      return_error: bool = False, *, method: Literal["pseudo", "qmc"] = "pseudo",
                      path_construction: Literal["bridge", "sequential"] = "bridge", scheme: Literal["euler", "qe"] = "euler"):
        """European prices on a strike x maturity grid from ONE set of paths: a float64 array (len(strikes), len(maturities)), the
        orientation of calibrate_heston's market_ivs[i, j]; with return_error, (prices, std_errors) of that shape.
        n_steps is the number of steps to the LONGEST maturity T = max(maturities), dt = T / n_steps; every maturity must lie on that
        grid: m = round(T_j / dt) with m >= 1 and |m dt - T_j| <= 1e-9 T, else ValueError naming the maturity, before the device is
        touched.  Maturities may come in any order and may repeat.  More than 16 cells are cut into launches of at most 16, sorted by
        step; each launch stops at its own last step and passes the same T, n_steps, seed and tables, and a cell's bits do not depend
        on the cells it shares a launch with.
        Ties: cell (K, T_j) is exp(-r T_j) mean(max(+-(spot[:, m_j] - K), 0)) over column m_j of
        simulate_paths(S, T, r, q, n_paths, n_steps, seed, method=..., path_construction=...)[0] (and of the mirrored paths with
        antithetic=True), its error exp(-r T_j) std / sqrt(samples) of the same payoffs -- which is what the reference's
        price_monte_carlo(S, K, T m/n, ..., n_paths, m, seed) computes cell by cell from one NumPy stream, its draws being per step.
        With method="pseudo" a cell on a grid where T m / n_steps is exact, e.g. T = 1 and n_steps = 64, has the sums of
        price_monte_carlo(S, K, T_j, ..., n_steps=m_j, seed=seed); the cell (K, T) always has those of price_monte_carlo(S, K, T, ...,
        n_steps, seed) for either method.
        With method="qmc" a cell at an INTERMEDIATE maturity is a read-out of the full-horizon construction (the Sobol dimensions and,
        for the bridge, the plan of n_steps dates): it is not the price price_monte_carlo(T_j, n_steps=m_j, method="qmc") would give,
        whose construction ends at T_j.  What the full-horizon construction buys at an intermediate date (the price scatter over
        scrambles against Philox seeds) has NOT been measured on the device yet: tools/heston_surface_timing.py measures it.
        seed=None, antithetic, method, path_construction, the standard error's meaning and the refusals as price_monte_carlo; also
        refused: empty strikes or maturities, a maturity <= 0.
        scheme as price_monte_carlo: with "qe" the cells are read-outs of simulate_paths(..., scheme="qe")'s columns in the same way
        (the launches, the ties to the matrix, the independence of the cells and the shards' sums all hold as above)."""
        qe = _check_scheme(scheme, method, path_construction)
        ks = _strike_list(strikes)
        _check_sizes(n_paths, n_steps)
        T, steps = _surface_steps(maturities, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        cells = _binding("surface", sobol, qe)
        return _fill_surface(ks, steps, lambda cell_k, cell_m: cells(S, T, r, q, option_type == "call", *self._model(), cell_k, cell_m, *run,
                                                                    antithetic), return_error)

    def _scenario_tuples(self, scenarios):
        """price_scenarios' mappings as _hip's tuples (S, K, T, r, q, is_call, kappa, theta, sigma_v, rho, v0), checked."""
        scenarios = list(scenarios)
        if not scenarios:
            raise ValueError("scenarios must not be empty")
        out = []
        for i, sc in enumerate(scenarios):
            missing = [key for key in ("S", "K", "T", "r") if key not in sc]
            if missing:
                raise ValueError(f"scenario {i} lacks {missing}")
            unknown = sorted(set(sc) - {"S", "K", "T", "r", "q", "option_type", *_SCENARIO_KEYS})
            if unknown:
                raise ValueError(f"scenario {i} has unknown keys {unknown}")
            T = float(sc["T"])
            if T <= 0.0:
                raise ValueError(f"scenario {i}: T must be > 0")
            model = [float(sc.get(key, getattr(self, key))) for key in _SCENARIO_KEYS]
            if not -1.0 <= model[3] <= 1.0:
                raise ValueError(f"scenario {i}: rho must be in [-1, 1]")
            out.append((float(sc["S"]), float(sc["K"]), T, float(sc["r"]), float(sc.get("q", 0.0)), sc.get("option_type", "call") == "call", *model))
        return out

    def price_scenarios(self, scenarios, n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False,
                        return_error: bool = False, *, method: Literal["pseudo", "qmc"] = "pseudo",
                        path_construction: Literal["bridge", "sequential"] = "bridge", scheme: Literal["euler", "qe"] = "euler"):
        """European prices under a list of what-if scenarios on COMMON random numbers: a float64 array (len(scenarios),), with
        return_error (prices, std_errors).  A scenario is a mapping with the keys S, K, T, r and optionally q (0), option_type
        ("call"; anything else prices as a put) and kappa, theta, sigma_v, rho, v0 (this pricer's own): spot, strike, maturity, rates
        and the model may all differ.  Scenario i is price_monte_carlo(S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic,
        method=..., path_construction=...) of a pricer with its model -- the same draws, the sums to rounding -- but the scenarios of a
        launch share ONE walk over the Philox blocks or Sobol points (and one fill of the two bridges): scenarios whose (T, kappa,
        theta, sigma_v, rho, v0) are equal as doubles share a path recursion, the others take one of their own on the same normals.
        The list is cut greedily, in the caller's order, into launches of at most 16 scenarios and at most 6 recursions; a scenario's
        bits depend neither on the cut nor on its neighbours nor on its place.  seed=None draws ONE seed for all launches.
        A scenario's v0 is not validated as HestonPricer's is: v0 < 0 means what it means at the C ABI (a deterministic first step).
        The scenarios run the Euler scheme; QE scenarios and Greeks are out of scope here.
        Refused (ValueError, before the device is touched): what price_monte_carlo refuses, an empty list, a scenario without S, K, T
        or r, with an unknown key, with T <= 0 or rho outside [-1, 1], and scheme="qe"."""
        _check_sizes(n_paths, n_steps)
        _check_euler_only(scheme, "price_scenarios")
        tuples = self._scenario_tuples(scenarios)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        prices = np.empty(len(tuples), dtype=np.float64)
        errors = np.empty_like(prices)
        for launch in _scenario_launches([_recursion_key(t[2], *t[6:]) for t in tuples]):
            sts = _binding("scenarios", sobol)([tuples[i] for i in launch], *run, antithetic)
            for i, st in zip(launch, sts):
                prices[i], errors[i] = st.price, st.std_error
        return (prices, errors) if return_error else prices

    def simulate_paths(self, S: float, T: float, r: float, q: float = 0.0, n_paths: int = 1000, n_steps: int = 252,
                       seed: Optional[int] = None, *, method: Literal["pseudo", "qmc"] = "pseudo",
                       path_construction: Literal["bridge", "sequential"] = "bridge",
                       scheme: Literal["euler", "qe"] = "euler") -> Tuple[np.ndarray, np.ndarray]:
        """heston.py:257-305: (spot_paths, variance_paths), each (n_paths, n_steps + 1), column 0 = (S, v0).
        The states of price_monte_carlo's recursion for the same seed, method, path_construction and scheme (additive, as there)."""
        _check_sizes(n_paths, n_steps)
        qe = _check_scheme(scheme, method, path_construction)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        return _binding("paths", sobol, qe)(S, T, r, q, *self._model(), *run, path_major=True)

    def _price_path_payoff(self, payoff: int, barrier: float, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error,
                           method, path_construction):
        """One launch of the path-payoff kernels (include/olmc.h "path payoffs under Heston") under price_monte_carlo's conventions."""
        _check_sizes(n_paths, n_steps)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        st = _binding("path_payoff", sobol)(S, K, T, r, q, option_type == "call", *self._model(), payoff, barrier, *run, antithetic)
        return _result(st, return_error)

    def price_asian(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                    avg_type: Literal["arithmetic", "geometric"] = "arithmetic", n_paths: int = 100000, n_steps: int = 252,
                    seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                    method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """The Asian option max(+-(A - K), 0) under this model, A the arithmetic or geometric mean of the spot over dates 1 .. n_steps: what
        AsianOption.price (exotic_options.py:97-131) computes from simulate_paths' spot matrix for the same seed, method and
        path_construction, in one launch that stores no path.  seed, antithetic, return_error, method and path_construction as
        price_monte_carlo: with method="qmc" the standard error is the naive per-path one, not a confidence interval (it overstates the
        error).  Refused (ValueError, before the device is touched): an unknown avg_type, and what price_monte_carlo refuses."""
        return self._price_path_payoff(_asian_payoff(avg_type), 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error, method,
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
        _check_barrier(barrier)
        return self._price_path_payoff(_barrier_kind(barrier_type), barrier, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic,
                                       return_error, method, path_construction)

    def price_lookback(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                       lookback_type: Literal["floating", "fixed"] = "floating", n_paths: int = 100000, n_steps: int = 252,
                       seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                       method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """The lookback option under this model on the extrema of simulate_paths' spot matrix over dates 0 .. n_steps: floating call S_n -
        S_min, floating put S_max - S_n, fixed call max(S_max - K, 0), fixed put max(K - S_min, 0) (LookbackOption.price,
        exotic_options.py:347-401), in one launch that stores no path.  The rest as price_asian; also refused: an unknown lookback_type."""
        return self._price_path_payoff(_lookback_payoff(lookback_type), 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error, method,
                                       path_construction)

    def price_american(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "put",
                       n_paths: int = 50000, n_steps: int = 50, poly_degree: int = 2, seed: Optional[int] = None, return_error: bool = False, *,
                       basis: Literal["spot_variance", "spot"] = "spot_variance", scheme: Literal["euler", "qe"] = "euler",
                       method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge"):
        """The American option under this model by Longstaff-Schwartz least-squares Monte Carlo (include/olha.h): AmericanOption.price's
        algorithm (exotic_options.py:259-306) on the matrices of simulate_paths(S, T, r, q, n_paths, n_steps, seed, method=...,
        path_construction=..., scheme=...), regressing at every exercise date 1 .. n_steps - 1 the discounted cash flows of the paths in
        the money on the date's state.  There is no antithetic mirror: the regression runs over the whole path set.
        basis: "spot_variance" (default) = all monomials x^a y^b, a + b <= poly_degree in [1, 3], of the standardised spot x and
        variance y (3, 6 or 10 unknowns) -- under stochastic volatility the continuation value depends on (S_t, v_t); "spot" = 1, x, ..,
        x^poly_degree, poly_degree in [1, 4], AmericanOption's one-factor fit on the Heston spot: a valid but lower price.  A date is
        fitted when more paths are in the money than the fit has unknowns; otherwise nobody exercises there.
        seed=None, return_error, method, path_construction and scheme as price_monte_carlo: with method="qmc" the standard error is the
        naive per-path one, and scheme="qe" takes path_construction="sequential" only.  T <= 0 returns the intrinsic value (error 0)
        without simulating.  Refused (ValueError, before the device is touched): an option_type other than "call" / "put", an unknown
        basis or scheme, poly_degree outside the basis's range, n_paths or n_steps < 1, and what price_monte_carlo refuses."""
        if option_type not in ("call", "put"):
            raise ValueError("option_type must be 'call' or 'put'")
        if basis not in ("spot_variance", "spot"):
            raise ValueError("basis must be 'spot_variance' or 'spot'")
        qe = _check_scheme(scheme, method, path_construction)
        top = 4 if basis == "spot" else 3
        if not 1 <= poly_degree <= top:
            raise ValueError(f"poly_degree must be in [1, {top}] for basis={basis!r}")
        _check_sizes(n_paths, n_steps)
        if T <= 0:
            intrinsic = max(S - K, 0) if option_type == "call" else max(K - S, 0)
            return (np.float64(intrinsic), 0.0) if return_error else np.float64(intrinsic)
        sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        entry = _hip.heston_american_lsm_qmc if sobol else _hip.heston_american_lsm
        return _result(entry(S, K, T, r, q, option_type == "call", *self._model(), *run, poly_degree, basis == "spot", qe), return_error)

    def _price_structured(self, philox, sobol, contract, S, T, r, q, n_paths, n_steps, seed, antithetic, return_error, method,
                          path_construction, scheme):
        """One launch of the structured-product kernels (include/olmc.h "structured products under Heston") under price_monte_carlo's
        conventions: `philox` / `sobol` are the product's two bindings, `contract` its arguments between the model and the counts."""
        qe = _check_scheme(scheme, method, path_construction)
        on_sobol, run = _draws(method, path_construction, n_paths, n_steps, seed)
        st = (sobol if on_sobol else philox)(S, T, r, q, *self._model(), *contract, *run, antithetic, qe=qe)
        return _result(st, return_error)

    def price_autocallable(self, S: float, T: float, r: float, q: float = 0.0, autocall_barrier: float = 1.0, coupon_barrier: float = 0.8,
                           coupon_rate: float = 0.10, ki_barrier: float = 0.6, observation_freq: int = 21, n_paths: int = 100000,
                           n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                           method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge",
                           scheme: Literal["euler", "qe"] = "euler"):
        """The autocallable note under this model, a fraction of notional: what AutocallableOption.price (exotic_options.py:438-491) computes
        from the spot matrix of simulate_paths(S, T, r, q, n_paths, n_steps, seed, method=..., path_construction=..., scheme=...), in one
        launch that stores no path.  The levels are relative to S; the observation dates are observation_freq, 2 observation_freq, ...
        <= n_steps; a payoff is discounted at its own date, so the price is the plain mean; the knock-in minimum includes date 0.
        observation_freq > n_steps leaves no observation date and every path runs to maturity: it is priced, as AutocallableOption prices
        it, with one observation on the last step at a level no path reaches.  The kernel decides in log space, ln(S_t / S) against
        ln(level): a path within rounding (about 1e-16 relative) of a level can decide differently from the matrix route.
        seed=None, antithetic, return_error, method, path_construction, scheme and the standard error's meaning as price_monte_carlo;
        scheme="qe" with method="qmc" takes path_construction="sequential" only.  A structured product's own grid (12 monthly resets, 4
        quarterly observations) is where "qe" matters: Euler on such a grid is biased by tens of standard errors (DESIGN.md "Structured
        products under Heston").  Refused (ValueError, before the device is touched): what price_monte_carlo refuses, and
        observation_freq < 1."""
        _check_sizes(n_paths, n_steps)
        if observation_freq < 1:
            raise ValueError("observation_freq must be >= 1")
        if observation_freq > n_steps:                  # no observation date: nothing redeems early (exotic_options.py:442, 448)
            observation_freq, autocall_barrier = n_steps, float("inf")
        contract = (autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq)
        return self._price_structured(_hip.heston_autocallable, _hip.heston_autocallable_qmc, contract, S, T, r, q, n_paths, n_steps, seed,
                                      antithetic, return_error, method, path_construction, scheme)

    def price_cliquet(self, S: float, T: float, r: float, q: float = 0.0, local_cap: float = 0.05, local_floor: float = -0.05,
                      global_cap: float = 0.30, global_floor: float = 0.0, n_periods: int = 12, n_paths: int = 100000, n_steps: int = 252,
                      seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False, *,
                      method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge",
                      scheme: Literal["euler", "qe"] = "euler"):
        """The cliquet under this model: exp(-r T) mean(max(clip(sum of clip(period return, local_floor, local_cap), global_floor,
        global_cap), 0) S) over n_periods periods of n_steps // n_periods steps from date 0 (trailing dates never enter a period) -- what
        CliquetOption.price (exotic_options.py:526-554) computes from simulate_paths' spot matrix for the same seed, method,
        path_construction and scheme, in one launch that stores no path.  The rest as price_autocallable; also refused: n_periods outside
        [1, n_steps]."""
        _check_sizes(n_paths, n_steps)
        if n_periods < 1 or n_periods > n_steps:
            raise ValueError("n_periods must be in [1, n_steps]")
        contract = (local_cap, local_floor, global_cap, global_floor, n_periods)
        return self._price_structured(_hip.heston_cliquet, _hip.heston_cliquet_qmc, contract, S, T, r, q, n_paths, n_steps, seed, antithetic,
                                      return_error, method, path_construction, scheme)


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


class HestonMCAdapter:
    """HestonAdapter's convention (sigma -> v0 = sigma^2, unified_greeks.py:74-104) over the device's own Monte Carlo price:
    ``price`` is price_monte_carlo of a COPY of the model with v0 = sigma^2 at the adapter's n_paths, n_steps, seed, antithetic, method
    and path_construction -- the wrapped pricer is never mutated -- so compute_greeks_unified(adapter, ...) differentiates the price
    price_monte_carlo gives.  seed=None draws one seed at construction: every bump sees the same random numbers, as
    MonteCarloPricer's do.  The adapter carries _fused_greeks, so compute_greeks_unified prices the 7 / 8 / 11 / 14 bumped contracts
    as ONE scenario launch of four recursions (olmc_heston_greeks_fd / olmc_heston_qmc_greeks_fd); fused=False goes the one launch
    per evaluation way and gives the same numbers to rounding.  Euler scheme only: QE Greeks are out of scope here.
    Refused (ValueError, before the device is touched): what price_monte_carlo refuses, and scheme="qe"."""

    def __init__(self, pricer: HestonPricer, n_paths: int = 100000, n_steps: int = 252, seed: Optional[int] = None, antithetic: bool = False, *,
                 method: Literal["pseudo", "qmc"] = "pseudo", path_construction: Literal["bridge", "sequential"] = "bridge",
                 scheme: Literal["euler", "qe"] = "euler"):
        _check_sizes(n_paths, n_steps)
        _check_euler_only(scheme, "HestonMCAdapter")
        self.heston = pricer
        self.n_paths, self.n_steps, self.antithetic = int(n_paths), int(n_steps), bool(antithetic)
        self.method, self.path_construction = method, path_construction
        self.seed = int(_seed(seed))
        self._qmc = _qmc_tables(method, path_construction, self.n_paths, self.n_steps, self.seed)      # the refusals, and the tables once

    def price(self, S, K, T, r, sigma, option_type, q=0.0, **kwargs) -> float:
        model = copy.copy(self.heston)
        model.v0 = sigma**2
        return model.price_monte_carlo(S, K, T, r, q, option_type, self.n_paths, self.n_steps, self.seed, self.antithetic,
                                       method=self.method, path_construction=self.path_construction, **kwargs)

    def _can_fuse(self, pricer_kwargs) -> bool:
        return not pricer_kwargs

    def _fused_greeks(self, S, K, T, r, sigma, option_type, q, include_second_order, seed=None):
        h = self.heston
        if self._qmc is not None:
            sv, shift, bridge = self._qmc
            vals, _ = _hip.heston_qmc_greeks_fd(S, K, T, r, sigma, q, option_type == "call", h.kappa, h.theta, h.sigma_v, h.rho, self.n_paths,
                                                sv, shift, bridge, self.antithetic, include_second_order, want_evals=False)
        else:
            vals, _ = _hip.heston_greeks_fd(S, K, T, r, sigma, q, option_type == "call", h.kappa, h.theta, h.sigma_v, h.rho, self.n_paths,
                                            self.n_steps, self.seed, self.antithetic, include_second_order, want_evals=False)
        keys = ("price", "delta", "gamma", "vega", "theta", "rho", "vanna", "charm", "vomma")
        return OrderedDict((k, np.float64(v)) for k, v in zip(keys if include_second_order else keys[:6], vals))


def greeks_heston_monte_carlo(heston_pricer, S: float, K: float, T: float, r: float, sigma: Optional[float] = None,
                              option_type: str = "call", q: float = 0.0, include_second_order: bool = True, **adapter_kwargs):
    """compute_greeks_unified over HestonMCAdapter(heston_pricer, **adapter_kwargs): the finite-difference Greeks of the Monte Carlo
    price in one launch.  sigma=None differentiates at the model's own start, sigma = sqrt(v0).  Euler scheme only."""
    from .greeks import compute_greeks_unified

    if sigma is None:
        sigma = float(np.sqrt(heston_pricer.v0))
    return compute_greeks_unified(HestonMCAdapter(heston_pricer, **adapter_kwargs), S, K, T, r, sigma, option_type, q, include_second_order)


def calibration_objective(market_data: dict, *, n_paths: int = 1 << 14, n_steps: Optional[int] = None, seed: int = 0,
                          method: Literal["pseudo", "qmc"] = "qmc", path_construction: Literal["bridge", "sequential"] = "bridge",
                          antithetic: bool = False, scheme: Literal["euler", "qe"] = "euler"):
    """calibrate_heston's objective as a function of (kappa, theta, sigma_v, rho, v0): checks market_data and the settings as
    calibrate_heston does (before the device is touched) and returns the callable; its attribute `evals` counts the surfaces priced.
    scheme as HestonPricer.price_surface; n_steps=None picks the grid as calibrate_heston does for the scheme."""
    from .black_scholes import implied_volatility

    missing = [key for key in ("spot", "strikes", "maturities", "market_ivs", "r") if key not in market_data]
    if missing:
        raise ValueError(f"market_data lacks {missing}")
    spot = float(market_data["spot"])
    strikes = np.asarray(market_data["strikes"], dtype=np.float64).ravel()
    maturities = np.asarray(market_data["maturities"], dtype=np.float64).ravel()
    market_ivs = np.asarray(market_data["market_ivs"], dtype=np.float64)
    r_rate = float(market_data["r"])
    q_yield = float(market_data.get("q", 0.0))
    if strikes.size == 0:
        raise ValueError("strikes must not be empty")
    _check_scheme(scheme, method, path_construction)
    if n_steps is None:
        n_steps = _grid_steps(maturities, _STEPS_PER_YEAR[scheme])
    _surface_steps(maturities, n_steps)
    if market_ivs.shape != (strikes.size, maturities.size):
        raise ValueError(f"market_ivs must have shape (len(strikes), len(maturities)) = {(strikes.size, maturities.size)}")
    if n_paths < 1:
        raise ValueError("n_paths and n_steps must be >= 1")
    if seed is None:
        raise ValueError("calibration needs a fixed seed: every objective evaluation must see the same random numbers")
    _qmc_tables(method, path_construction, n_paths, n_steps, seed)         # price_surface's refusals, once and ahead of the optimiser
    quoted = ~np.isnan(market_ivs)

    def objective(params):
        kappa, theta, sigma_v, rho, v0 = (float(p) for p in params)
        if kappa <= 0 or theta <= 0 or sigma_v <= 0 or v0 <= 0:
            return 1e10
        if not -0.99 <= rho <= 0.99:
            return 1e10
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)        # Feller, at every trial point
                pricer = HestonPricer(kappa, theta, sigma_v, rho, v0)
        except ValueError:
            return 1e10
        objective.evals += 1
        prices = pricer.price_surface(spot, strikes, maturities, r_rate, q_yield, "call", n_paths, n_steps, seed, antithetic,
                                      method=method, path_construction=path_construction, scheme=scheme)
        total, count = 0.0, 0
        for i, K in enumerate(strikes):
            for j, T in enumerate(maturities):
                if not quoted[i, j]:
                    continue
                try:
                    total += (implied_volatility(float(prices[i, j]), spot, float(K), float(T), r_rate, "call", q_yield) - market_ivs[i, j]) ** 2
                except ValueError:
                    total += 1.0                                    # heston.py:383-385
                count += 1
        return total / max(count, 1)

    objective.evals = 0
    return objective


def calibrate_heston(market_data: dict, initial_params: Optional[dict] = None, *, n_paths: int = 1 << 14, n_steps: Optional[int] = None,
                     seed: int = 0, method: Literal["pseudo", "qmc"] = "qmc", path_construction: Literal["bridge", "sequential"] = "bridge",
                     antithetic: bool = False, maxiter: int = 200, scheme: Literal["euler", "qe"] = "euler") -> HestonPricer:
    """heston.py:312-414 on the device's own Monte Carlo prices: fit (kappa, theta, sigma_v, rho, v0) to an implied-volatility surface.

    market_data: spot, strikes, maturities, market_ivs[i, j] (strike i, maturity j; NaN = no quote), r and optionally q.  As in the
    reference: the default start (2.0, 0.04, 0.3, -0.5, 0.04), L-BFGS-B with its bounds and maxiter=200, the objective = the mean squared
    difference of model and market implied volatility over the quoted cells, 1e10 outside the bounds, +1.0 for a cell whose model
    implied volatility cannot be found.  Unlike the reference, whose objective prices with the semi-analytic price_european, the model
    prices here come from ONE price_surface per objective evaluation (calls, the given n_paths, method, path_construction, antithetic)
    at a FIXED seed: every evaluation sees the same random numbers, so the objective is a deterministic function of the five parameters,
    and the model is calibrated to the pricer price_monte_carlo and price_surface are.
    n_steps=None picks the smallest grid with at least 64 steps per year to the longest maturity on which every maturity lies
    (ValueError if none of at most 1024 steps exists).  Returns the calibrated HestonPricer with the final objective value and the number
    of surfaces priced (objective evaluations inside the bounds) attached as `calibration_error` and `calibration_evals`.  maxiter
    (additive) caps L-BFGS-B's iterations; the default is the reference's 200.
    scheme (additive) as HestonPricer.price_surface: "qe" calibrates on the quadratic-exponential scheme's surfaces, with
    method="qmc" (the default here) on path_construction="sequential" only -- the default "bridge" is refused; n_steps=None then picks
    at least 16 steps per year instead of 64.  At a model that violates the Feller condition Euler's bias at 16-64 steps per year is
    tens of standard errors (DESIGN.md "Heston: the quadratic-exponential scheme"), so Euler's objective at the parameters that
    generated a surface is far from 0 and QE's is not.
    Refused (ValueError, before the device is touched): a missing market_data key, market_ivs of another shape than
    (len(strikes), len(maturities)), seed=None, and what price_surface refuses."""
    from scipy.optimize import minimize

    objective = calibration_objective(market_data, n_paths=n_paths, n_steps=n_steps, seed=seed, method=method,
                                      path_construction=path_construction, antithetic=antithetic, scheme=scheme)
    if initial_params is None:
        initial_params = {"kappa": 2.0, "theta": 0.04, "sigma_v": 0.3, "rho": -0.5, "v0": 0.04}
    x0 = [initial_params[key] for key in ("kappa", "theta", "sigma_v", "rho", "v0")]
    bounds = [(0.01, 10.0), (0.001, 1.0), (0.01, 2.0), (-0.99, 0.99), (0.001, 1.0)]
    result = minimize(objective, x0, method="L-BFGS-B", bounds=bounds, options={"maxiter": maxiter})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        pricer = HestonPricer(*(float(p) for p in result.x))
    pricer.calibration_error = float(result.fun)
    pricer.calibration_evals = objective.evals
    return pricer
