"""What the path pricers of heston.py, local_vol.py, jump_diffusion.py and exotic.py share below their public methods: the seed draw,
the (price, error) result, the size check, the payoff vocabulary and the strike x maturity surface.  Private; imports only _hip and
NumPy.  Every refusal here is a ValueError raised before the library is loaded, and the callers' order of refusals is part of their
behaviour: a helper judges exactly what its name says and nothing else.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import _hip

_SURFACE_CELLS = 16          # cells of one launch (OLMC_MAX_BATCH)


def _seed(seed: Optional[int]) -> int:
    """The seed itself, or one fresh 31-bit draw for seed=None: callers draw once per call, and once for all launches of a call."""
    return seed if seed is not None else int(np.random.default_rng().integers(0, 2**31))


def _result(st, return_error: bool):
    return (np.float64(st.price), float(st.std_error)) if return_error else np.float64(st.price)


def _check_sizes(n_paths: int, n_steps: int) -> None:
    if n_paths < 1 or n_steps < 1:
        raise ValueError("n_paths and n_steps must be >= 1")


def _asian_payoff(avg_type: str) -> int:
    if avg_type not in ("arithmetic", "geometric"):
        raise ValueError("avg_type must be 'arithmetic' or 'geometric'")
    return _hip.PATH_ASIAN_GEOMETRIC if avg_type == "geometric" else _hip.PATH_ASIAN_ARITHMETIC


def _check_barrier(barrier: float) -> None:
    if barrier <= 0:                       # exotic_options.py:195-196
        raise ValueError("Barrier must be positive")


def _barrier_kind(barrier_type: str) -> int:
    """The BARRIER_KINDS value of barrier_type, read as the reference's class reads it (exotic_options.py:201-212): startswith("up")
    and endswith("out")."""
    return (0 if barrier_type.startswith("up") else 2) + (0 if barrier_type.endswith("out") else 1)


def _lookback_payoff(lookback_type: str) -> int:
    if lookback_type not in ("floating", "fixed"):
        raise ValueError("lookback_type must be 'floating' or 'fixed'")
    return _hip.LOOKBACK_FIXED if lookback_type == "fixed" else _hip.LOOKBACK_FLOATING


def _strike_list(strikes) -> list:
    ks = [float(k) for k in np.asarray(strikes, dtype=np.float64).ravel()]
    if not ks:
        raise ValueError("strikes must not be empty")
    return ks


def _surface_steps(maturities, n_steps: int) -> Tuple[float, list]:
    """(T, the grid step of every maturity): T = max(maturities), dt = T / n_steps, maturity T_j sits at step m = round(T_j / dt) and
    must lie on the grid (m >= 1, |m dt - T_j| <= 1e-9 T).  ValueError names the maturity that does not."""
    mats = [float(t) for t in np.asarray(maturities, dtype=np.float64).ravel()]
    if not mats:
        raise ValueError("maturities must not be empty")
    for t in mats:
        if not t > 0.0:                                   # NaN included
            raise ValueError(f"maturity {t!r} must be > 0")
    if n_steps < 1:
        raise ValueError("n_paths and n_steps must be >= 1")
    T = max(mats)
    dt = T / n_steps
    steps = []
    for t in mats:
        m = int(round(t / dt))
        if m < 1 or m > n_steps or abs(m * dt - t) > 1e-9 * T:
            raise ValueError(f"maturity {t!r} is not on the grid of {n_steps} steps to T = {T!r} (dt = {dt!r})")
        steps.append(m)
    return T, steps


def _surface_launches(steps, n_strikes: int):
    """The cells (i, j) = (strike index, maturity index) of a surface cut into launches: sorted by step (then maturity index, then
    strike index), at most 16 cells each -- every cell once; a launch's step loop ends at its own last step."""
    cells = sorted(((steps[j], j, i) for j in range(len(steps)) for i in range(n_strikes)))
    return [[(i, j) for _m, j, i in cells[a:a + _SURFACE_CELLS]] for a in range(0, len(cells), _SURFACE_CELLS)]


def _grid_steps(maturities, per_year: int = 64, cap: int = 1024) -> int:
    """The smallest n_steps <= cap with at least per_year steps per year to the longest maturity on whose grid every maturity lies."""
    mats = [float(t) for t in np.asarray(maturities, dtype=np.float64).ravel()]
    if not mats or not all(t > 0.0 for t in mats):
        raise ValueError("maturities must be a non-empty list of positive times")
    T = max(mats)
    for n in range(max(1, int(np.ceil(per_year * T - 1e-9))), cap + 1):
        try:
            _surface_steps(mats, n)
        except ValueError:
            continue
        return n
    raise ValueError(f"no grid of at most {cap} steps to T = {T!r} holds every maturity of {mats!r}: pass n_steps, or move the maturities")


def _fill_surface(ks, steps, launch, return_error: bool):
    """prices[i, j] (and the errors) of the cells (ks[i], steps[j]), launch by launch: launch(cell_strikes, cell_steps) -> [Stats] prices at
    most 16 cells, and every launch of one surface is given the same seed or tables by its caller."""
    prices = np.empty((len(ks), len(steps)), dtype=np.float64)
    errors = np.empty_like(prices)
    for cut in _surface_launches(steps, len(ks)):
        sts = launch([ks[i] for i, _j in cut], [steps[j] for _i, j in cut])
        for (i, j), st in zip(cut, sts):
            prices[i, j], errors[i, j] = st.price, st.std_error
    return (prices, errors) if return_error else prices
