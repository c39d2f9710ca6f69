"""Closed-form European price under Black-Scholes-Merton with a continuous yield.

The accuracy anchor of every Monte Carlo test, as in the reference
(src/pricing_models/black_scholes.py:9-52: same argument order, ValueError on
S <= 0, K <= 0, T < 0 or sigma < 0, and T == 0 -> intrinsic value).  Scalar host
arithmetic, written on the forward: C = D (F N(d+) - K N(d-)), P = D (K N(-d-) - F N(-d+)).

`implied_volatility` inverts it (the behaviour of src/pricing_models/iv_solver.py:65-159).
"""
import math

_SQRT2 = math.sqrt(2.0)


def _ncdf(x: float) -> float:
    """Standard normal CDF via erfc (no SciPy dependency; 1e-16 of scipy.stats.norm.cdf)."""
    return 0.5 * math.erfc(-x / _SQRT2)


def black_scholes(S, K, T, r, sigma, option_type="call", q=0.0):
    bad = [name for name, ok in (("S", S > 0), ("K", K > 0), ("T", T >= 0), ("sigma", sigma >= 0)) if not ok]
    if bad:
        raise ValueError("Invalid input: all inputs must be positive, and T, sigma >= 0")
    is_call = option_type == "call"
    if not is_call and option_type != "put":
        if T == 0:       # the reference prices anything at expiry before checking the type
            return max(K - S, 0.0)
        raise ValueError("option_type must be 'call' or 'put'")
    if T == 0:
        return max(S - K, 0.0) if is_call else max(K - S, 0.0)
    total_vol = sigma * math.sqrt(T)
    carry = math.exp(-q * T)                 # spot leg discounting
    discount = math.exp(-r * T)              # strike leg discounting
    d_plus = (math.log(S / K) + (r - q + 0.5 * sigma**2) * T) / total_vol
    d_minus = d_plus - total_vol
    if is_call:
        return S * carry * _ncdf(d_plus) - K * discount * _ncdf(d_minus)
    return K * discount * _ncdf(-d_minus) - S * carry * _ncdf(-d_plus)


def implied_volatility(price, S, K, T, r, option_type="call", q=0.0, *, tolerance=1e-8, bounds=(0.001, 5.0)):
    """The volatility in `bounds` at which black_scholes(S, K, T, r, sigma, option_type, q) equals `price`.

    What the reference's solver (iv_solver.py:65-159) refuses is refused here, with ValueError: price <= 0; S, K or T <= 0; a price
    more than `tolerance` below the discounted intrinsic value max(+-(S e^{-qT} - K e^{-rT}), 0); a price that the volatilities
    0.1 % and 500 % (the reference's bounds) do not bracket.  The reference runs Newton's method from 0.2 and returns the first
    iterate whose PRICE is within `tolerance` (1e-8) of the target, falling back on Brent's method between the bounds; here the
    root is bracketed between the bounds from the start (Brent's method on this module's black_scholes) and located to the precision
    the price allows, so the answer does not depend on a starting point: the two agree to tolerance / vega."""
    from scipy.optimize import brentq

    if not price > 0:
        raise ValueError("Market price must be positive")
    if not (S > 0 and K > 0 and T > 0):
        raise ValueError("S, K, T must be positive")
    if option_type not in ("call", "put"):
        raise ValueError("option_type must be 'call' or 'put'")
    forward_leg, strike_leg = S * math.exp(-q * T), K * math.exp(-r * T)
    intrinsic = max(forward_leg - strike_leg, 0.0) if option_type == "call" else max(strike_leg - forward_leg, 0.0)
    if price < intrinsic - tolerance:
        raise ValueError(f"Price {price:.4f} below intrinsic value {intrinsic:.4f}")

    def miss(sigma):
        return black_scholes(S, K, T, r, sigma, option_type, q) - price

    low, high = miss(bounds[0]), miss(bounds[1])
    if low > 0:
        raise ValueError(f"Could not find implied volatility: Price too low for IV computation (below {bounds[0] * 100:.1f}% vol)")
    if high < 0:
        raise ValueError(f"Could not find implied volatility: Price too high for IV computation (above {bounds[1] * 100:.1f}% vol)")
    if low == 0:
        return float(bounds[0])
    if high == 0:
        return float(bounds[1])
    return float(brentq(miss, bounds[0], bounds[1], xtol=1e-14, rtol=8.9e-16, maxiter=200))
