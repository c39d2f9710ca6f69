"""DupireLocalVol on the device path engine (reference: src/pricing_models/local_vol.py).

Calibration follows the reference's rules in code of this package's own: `dupire_formula` (:73-138) as whole-grid NumPy, `calibrate`
(:140-179) on the same SciPy spline, floors, fallbacks and fills included, tied to the reference by tests/golden/local_vol.json.  Pricing is new: where the reference's
`price_fdm` (:181-262) runs an explicit finite-difference loop in Python for one vanilla, the calibrated surface is sampled into a
uniform table over (tau, x = ln(S_t / S)) (`local_vol_table`) and Monte Carlo paths walk it on the GPU (include/olmc_local_vol.h):
Europeans, Asians, barriers, lookbacks and a strike x maturity surface, each in one launch, on the GBM Philox stream.
`price_fdm` itself is not restated (INTEGRATION.md "Local volatility").
Additive: `DupireLocalVolQMC` (`model.qmc()`) runs the same methods on scrambled-Sobol points (include/olmc_local_vol_qmc.h).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Literal, Optional, Tuple

import numpy as np

from . import _hip
from ._paths import _asian_payoff, _barrier_kind, _check_barrier, _check_sizes, _fill_surface, _lookback_payoff, _result, _seed, _strike_list, _surface_steps

_VOL_CLIP = (0.05, 2.0)          # local_vol.py:238
_SAMPLE_EXPIRIES = (0.1, 0.25, 0.5, 0.75, 1.0)
_FLAT_VOL = 0.2                  # the reference's fallback without a calibrated surface (:207-209)


_VARIANCE_FLOOR = 0.001          # Dupire's ratio is floored here before the square root
_CONVEXITY_MIN = 1e-10           # K^2 d2C/dK2 at or below this: no usable convexity, the cell keeps its implied volatility


@dataclass
class LocalVolSurface:
    """A calibrated local-volatility surface: the node matrix values[len(expiries), len(strikes)] and, when there are enough nodes for
    one, an interpolator(K, T).  Field names and call signature are those of the reference's class, so its users can switch."""

    strikes: np.ndarray
    expiries: np.ndarray
    values: np.ndarray
    spot: float
    interpolator: Optional[Callable] = None

    def __call__(self, K: float, T: float) -> float:
        """sigma_local(K, T).  Without an interpolator (a single strike or expiry): piecewise linear in K over column 0 of the matrix."""
        evaluate = self.interpolator
        if evaluate is None:
            first_column = self.values[:, 0]
            return np.interp(K, self.strikes, first_column)
        return float(evaluate(K, T))


def _call_grid(spot: float, strikes: np.ndarray, expiries: np.ndarray, vols: np.ndarray, r: float, q: float) -> np.ndarray:
    """Black-Scholes call prices on the whole (expiry, strike) grid at once; an expiry <= 0 prices at intrinsic value."""
    from scipy.special import ndtr

    k = np.asarray(strikes, dtype=np.float64)[None, :]
    t = np.asarray(expiries, dtype=np.float64)[:, None]
    live = t > 0
    tt = np.where(live, t, 1.0)
    sd = vols * np.sqrt(tt)
    d_plus = (np.log(spot / k) + (r - q + 0.5 * vols**2) * tt) / sd
    priced = spot * np.exp(-q * tt) * ndtr(d_plus) - k * np.exp(-r * tt) * ndtr(d_plus - sd)
    return np.where(live, priced, np.maximum(spot - k, 0.0))


class DupireLocalVol:
    """Dupire local volatility: calibrated by the reference's rules, priced on Monte Carlo paths under sigma(S, t).

    n_paths, n_steps and seed (keyword-only, additive) are the sizes `price` runs with and the defaults of every pricing method; with
    seed=None every call draws a seed of its own, so finite-difference Greeks through `price` want a fixed seed."""

    def __init__(self, r: float = 0.05, q: float = 0.0, *, n_paths: int = 100_000, n_steps: int = 252, seed: Optional[int] = None):
        self.r = r
        self.q = q
        self.n_paths = n_paths
        self.n_steps = n_steps
        self.seed = seed
        self._calibrated: Optional[LocalVolSurface] = None
        self._spline = None

    def dupire_formula(self, strikes: np.ndarray, expiries: np.ndarray, iv_surface: np.ndarray, spot: float) -> np.ndarray:
        """sigma_local^2(K, T) = 2 (dC/dT + (r - q) K dC/dK + q C) / (K^2 d2C/dK2) on the whole grid at once, with the rules
        tests/golden/local_vol.json pins to the reference: a backward difference in T and central differences in K, both over the MEAN
        node spacing (0.01 in T for a single expiry); the ratio floored at 0.001 under the root; the cell's implied volatility where
        the convexity term is not above 1e-10; the first expiry's row is the implied volatilities, and the two outer strike columns
        repeat their neighbours (after the first row is set)."""
        vols = np.asarray(iv_surface, dtype=np.float64)
        k = np.asarray(strikes, dtype=np.float64)
        t = np.asarray(expiries, dtype=np.float64)
        calls = _call_grid(spot, k, t, vols, self.r, self.q)
        h_k = np.diff(k).mean()
        h_t = np.diff(t).mean() if t.size > 1 else 0.01
        here, left, right = calls[1:, 1:-1], calls[1:, :-2], calls[1:, 2:]          # rows 1.., the interior strikes and their neighbours
        k_in = k[1:-1][None, :]
        in_time = (here - calls[:-1, 1:-1]) / h_t
        in_strike = (right - left) / (2 * h_k)
        convexity = k_in**2 * ((right - 2 * here + left) / h_k**2)
        twice_drift = 2 * (in_time + (self.r - self.q) * k_in * in_strike + self.q * here)
        usable = convexity > _CONVEXITY_MIN
        ratio = np.divide(twice_drift, convexity, out=np.zeros_like(here), where=usable)
        sigma = np.array(vols, copy=True)                                         # row 0 and the unusable cells stay implied volatilities
        sigma[1:, 1:-1] = np.where(usable, np.sqrt(np.maximum(ratio, _VARIANCE_FLOOR)), vols[1:, 1:-1])
        sigma[:, 0], sigma[:, -1] = sigma[:, 1], sigma[:, -2]
        return sigma

    def calibrate(self, strikes: np.ndarray, expiries: np.ndarray, iv_surface: np.ndarray, spot: float) -> LocalVolSurface:
        """dupire_formula's matrix behind a bicubic spline over (strike, expiry), as the reference builds it: SciPy's
        RectBivariateSpline, which holds the surface flat outside its nodes and needs four nodes each way.  A single strike or expiry
        gets no interpolator.  The surface is kept for the pricing methods and returned."""
        sigma = self.dupire_formula(strikes, expiries, iv_surface, spot)
        spline = evaluate = None
        if min(len(strikes), len(expiries)) > 1:
            from scipy.interpolate import RectBivariateSpline

            spline = RectBivariateSpline(strikes, expiries, sigma.T, kx=3, ky=3)
            evaluate = lambda K, T: float(spline(K, T)[0, 0])  # noqa: E731
        self._spline = spline
        self._calibrated = LocalVolSurface(strikes=strikes, expiries=expiries, values=sigma, spot=spot, interpolator=evaluate)
        return self._calibrated

    # ------------------------------------------------------------------ the device table ----
    def local_vol_table(self, S: float, T: float, n_x: int = 128, n_t: int = 33) -> Tuple[np.ndarray, float, float, float]:
        """(vol[n_t][n_x], x_lo, x_hi, t_hi): the calibrated surface sigma(K = S e^x, tau), clipped to [0.05, 2.0] as local_vol.py:238 clips
        it, on the uniform grid the kernels read (include/olmc_local_vol.h): columns x_j from ln(K_first / S) to ln(K_last / S), rows
        tau_i = i t_hi / (n_t - 1) from 0 to t_hi = min(T, the last expiry).  The kernels hold the table flat beyond its edges and the
        reference's spline holds the surface flat outside its nodes, so beyond the strikes' range and after the last expiry the two mean
        the same thing; rows before the first expiry carry the spline's flat extension.  Uncalibrated: a flat 0.2, the reference's
        fallback (:207-209)."""
        if n_x < 2 or n_t < 1:
            raise ValueError("n_x must be >= 2 and n_t >= 1")
        if self._calibrated is None:
            return np.full((1, 2), _FLAT_VOL), -1.0, 1.0, 1.0
        sf = self._calibrated
        x_lo, x_hi = float(np.log(sf.strikes[0] / S)), float(np.log(sf.strikes[-1] / S))
        t_hi = float(min(T, sf.expiries[-1])) if n_t > 1 else 1.0
        ks = S * np.exp(np.linspace(x_lo, x_hi, n_x))
        ks[0], ks[-1] = sf.strikes[0], sf.strikes[-1]                        # the end columns sit on the end nodes, not an ulp beside them
        ts = np.linspace(0.0, t_hi, n_t) if n_t > 1 else np.array([float(min(T, sf.expiries[-1]))])
        if self._spline is not None and sf.interpolator is not None:
            vol = np.asarray(self._spline(ks, ts)).T                         # the grid form of interpolator(K, T), node by node
        else:
            vol = np.array([[float(sf(k, t)) for k in ks] for t in ts])
        return np.clip(vol, *_VOL_CLIP), x_lo, x_hi, t_hi

    # ------------------------------------------------------------------ pricing ----
    def _sizes(self, n_paths, n_steps, seed):
        n_paths = self.n_paths if n_paths is None else n_paths
        n_steps = self.n_steps if n_steps is None else n_steps
        _check_sizes(n_paths, n_steps)
        return n_paths, n_steps, _seed(self.seed if seed is None else seed)

    # The three device calls, each on a table of local_vol_table and the sizes and seed _sizes settled: what DupireLocalVolQMC overrides.
    def _device_price(self, S, K, T, r, q, is_call, table, payoff, barrier, n_paths, n_steps, seed, antithetic):
        return _hip.lv_price(S, K, T, r, q, is_call, table, payoff, barrier, n_paths, n_steps, seed, antithetic)

    def _device_paths(self, S, T, r, q, table, n_paths, n_steps, seed):
        return _hip.lv_paths(S, T, r, q, table, n_paths, n_steps, seed, path_major=True)

    def _device_surface(self, S, T, r, q, is_call, table, strikes, steps, n_paths, n_steps, seed, antithetic):
        return _hip.lv_surface_prices(S, T, r, q, is_call, table, strikes, steps, n_paths, n_steps, seed, antithetic)

    def _price_payoff(self, payoff, barrier, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error):
        n_paths, n_steps, s = self._sizes(n_paths, n_steps, seed)
        st = self._device_price(S, K, T, r, q, option_type == "call", self.local_vol_table(S, T), payoff, barrier, n_paths, n_steps, s, antithetic)
        return _result(st, return_error)

    def price_monte_carlo(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                          n_paths: Optional[int] = None, n_steps: Optional[int] = None, seed: Optional[int] = None, antithetic: bool = False,
                          return_error: bool = False):
        """exp(-r T) mean(max(+-(S_n - K), 0)) over paths of x_{t+1} = x_t + (r - q - sigma_t^2 / 2) dt + sigma_t sqrt(dt) z_t, S_t = S
        exp(x_t), sigma_t = the table of local_vol_table(S, T) at (x_t, t dt): one launch that stores no path.  The paths are
        simulate_paths' rows for the same seed.  n_paths, n_steps, seed: None takes the constructor's.  antithetic also walks the mirrored
        path -z, under its own volatilities (2 n_paths samples).  Anything but "call" prices as a put."""
        return self._price_payoff(_hip.LV_EUROPEAN, 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def simulate_paths(self, S: float, T: float, r: float, q: float = 0.0, n_paths: int = 1000, n_steps: int = 252,
                       seed: Optional[int] = None) -> np.ndarray:
        """The spot matrix (n_paths, n_steps + 1) of price_monte_carlo's recursion for the same seed; column 0 is S itself."""
        n_paths, n_steps, s = self._sizes(n_paths, n_steps, seed)
        return self._device_paths(S, T, r, q, self.local_vol_table(S, T), n_paths, n_steps, s)

    def price_asian(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                    avg_type: Literal["arithmetic", "geometric"] = "arithmetic", n_paths: Optional[int] = None, n_steps: Optional[int] = None,
                    seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False):
        """max(+-(A - K), 0), A the arithmetic or geometric mean of simulate_paths' spot over dates 1 .. n_steps (HestonPricer.price_asian's
        payoff), on local-volatility paths."""
        return self._price_payoff(_asian_payoff(avg_type), 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_barrier(self, S: float, K: float, T: float, r: float, barrier: float, q: float = 0.0,
                      option_type: Literal["call", "put"] = "call",
                      barrier_type: Literal["up-and-out", "up-and-in", "down-and-out", "down-and-in"] = "up-and-out",
                      n_paths: Optional[int] = None, n_steps: Optional[int] = None, seed: Optional[int] = None, antithetic: bool = False,
                      return_error: bool = False):
        """The barrier option monitored at dates 0 .. n_steps of simulate_paths' matrix, with HestonPricer.price_barrier's reading of
        barrier_type, its date-0 decision and its log-space comparison after date 0.  Refused: barrier <= 0."""
        _check_barrier(barrier)
        return self._price_payoff(_barrier_kind(barrier_type), barrier, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_lookback(self, S: float, K: float, T: float, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                       lookback_type: Literal["floating", "fixed"] = "floating", n_paths: Optional[int] = None, n_steps: Optional[int] = None,
                       seed: Optional[int] = None, antithetic: bool = False, return_error: bool = False):
        """The lookback option on the extrema of simulate_paths' matrix over dates 0 .. n_steps (HestonPricer.price_lookback's payoffs)."""
        return self._price_payoff(_lookback_payoff(lookback_type), 0.0, S, K, T, r, q, option_type, n_paths, n_steps, seed, antithetic, return_error)

    def price_surface(self, S: float, strikes, maturities, r: float, q: float = 0.0, option_type: Literal["call", "put"] = "call",
                      n_paths: Optional[int] = None, n_steps: Optional[int] = None, seed: Optional[int] = None, antithetic: bool = False,
                      return_error: bool = False):
        """European prices on a strike x maturity grid from ONE set of paths: an array (len(strikes), len(maturities)), with return_error
        (prices, std_errors).  The grid, its refusals and the launches of at most 16 cells are HestonPricer.price_surface's: n_steps steps
        to the longest maturity, every maturity on that grid; cell (K, T_j) is the discounted payoff of column m_j of simulate_paths'
        matrix.  This is the call that reprices a whole smile."""
        ks = _strike_list(strikes)
        n_paths, n_steps, s = self._sizes(n_paths, n_steps, seed)
        T, steps = _surface_steps(maturities, n_steps)
        table = self.local_vol_table(S, T)
        return _fill_surface(ks, steps, lambda cell_k, cell_m: self._device_surface(S, T, r, q, option_type == "call", table, cell_k, cell_m, n_paths,
                                                                                   n_steps, s, antithetic), return_error)

    def price(self, S: float, K: float, T: float, r: float, sigma: float, option_type: str, q: float = 0.0) -> float:
        """PricerProtocol (local_vol.py:264-277): sigma is ignored, the calibrated surface prices; r and q are kept, as the reference keeps
        them.  price_monte_carlo with the constructor's n_paths, n_steps and seed: compute_greeks_unified(model, ...) works as it stands,
        one launch per bump -- under common random numbers when the constructor was given a seed."""
        self.r = r
        self.q = q
        return float(self.price_monte_carlo(S, K, T, r, q, option_type))

    def qmc(self, path_construction: Literal["bridge", "sequential"] = "bridge") -> "DupireLocalVolQMC":
        """This model on scrambled-Sobol points: a view that shares the calibrated surface and spline objects and takes r, q, n_paths,
        n_steps and seed as they are now."""
        view = DupireLocalVolQMC(self.r, self.q, n_paths=self.n_paths, n_steps=self.n_steps, seed=self.seed, path_construction=path_construction)
        view._calibrated, view._spline = self._calibrated, self._spline
        return view


class DupireLocalVolQMC(DupireLocalVol):
    """DupireLocalVol on scrambled-Sobol paths (include/olmc_local_vol_qmc.h): every pricing method, simulate_paths, price_surface and
    price keep their signatures and meanings; n_paths counts Sobol points and path i is point i of scipy.stats.qmc.Sobol(d = n_steps,
    scramble=True, seed), one dimension per step.  path_construction="bridge" (the default, at most 1024 steps) builds the Brownian
    path by the breadth-first bridge and steps on its increments, "sequential" gives step t dimension t (at most 21201 steps).  The
    refusals are exotic._qmc_tables', ValueErrors raised before the device is touched.  return_error's figure is the naive standard
    error of the payoffs: for Sobol points it overstates the error.  With seed=None every call draws a scramble of its own; with a
    fixed seed compute_greeks_unified(model.qmc(), ...) differentiates on the same points, one launch per bump."""

    def __init__(self, r: float = 0.05, q: float = 0.0, *, n_paths: int = 1 << 14, n_steps: int = 252, seed: Optional[int] = None,
                 path_construction: Literal["bridge", "sequential"] = "bridge"):
        if path_construction not in ("bridge", "sequential"):
            raise ValueError("path_construction must be 'bridge' or 'sequential'")
        super().__init__(r, q, n_paths=n_paths, n_steps=n_steps, seed=seed)
        self.path_construction = path_construction

    def _sobol(self, n_paths, n_steps, seed):
        """(sv, shift, bridge) of Sobol(d = n_steps, seed); sobol_tables caches them, so price_surface's launches share one pair."""
        from .exotic import _qmc_tables

        return _qmc_tables("qmc", self.path_construction, n_paths, n_steps, seed)

    def _device_price(self, S, K, T, r, q, is_call, table, payoff, barrier, n_paths, n_steps, seed, antithetic):
        sv, shift, bridge = self._sobol(n_paths, n_steps, seed)
        return _hip.lvq_price(S, K, T, r, q, is_call, table, payoff, barrier, n_paths, sv, shift, bridge, antithetic)

    def _device_paths(self, S, T, r, q, table, n_paths, n_steps, seed):
        sv, shift, bridge = self._sobol(n_paths, n_steps, seed)
        return _hip.lvq_paths(S, T, r, q, table, n_paths, sv, shift, bridge, path_major=True)

    def _device_surface(self, S, T, r, q, is_call, table, strikes, steps, n_paths, n_steps, seed, antithetic):
        sv, shift, bridge = self._sobol(n_paths, n_steps, seed)
        return _hip.lvq_surface_prices(S, T, r, q, is_call, table, strikes, steps, n_paths, sv, shift, bridge, antithetic)


def create_sample_iv_surface(spot: float = 100, n_strikes: int = 20, n_expiries: int = 5) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(strikes, expiries, iv_surface[len(expiries), len(strikes)]): the reference's sample market.  Strikes run evenly from 70 % to
    130 % of spot, the expiries are the first n_expiries of 0.1, 0.25, 0.5, 0.75, 1; the at-the-money level is 0.20 + 0.05 sqrt(T), and
    a quadratic smile in log-moneyness m, 0.1 m^2 - 0.05 m, flattens with sqrt(0.25 / T)."""
    strikes = np.linspace(0.7 * spot, 1.3 * spot, n_strikes)
    expiries = np.asarray(_SAMPLE_EXPIRIES[:n_expiries], dtype=np.float64)
    m = np.log(strikes / spot)[None, :]
    term = expiries[:, None]
    return strikes, expiries, (0.20 + 0.05 * np.sqrt(term)) + (0.1 * m**2 - 0.05 * m) * np.sqrt(0.25 / term)
