"""The SABR path matrices on scrambled-Sobol points as an extended-precision recursion (not a test module).

include/olmc_sabr_qmc.h restated from outside the device: the normals of SciPy's Sobol(d = 2n, scramble=True, seed) through
tests/sobol_reference.normal_chunks, Heston's dimension assignment (sequential: dimensions 2t, 2t + 1 are Z1, Z2' of step t; bridge:
W1 on the even and W2 on the odd dimensions of the breadth-first plan, step t taking their increments), and olmc_sabr.h's recursion
in np.longdouble on these TRUE normals (no sqrt(2 ln 2) scale), on the constants the host folds in fp64 (dt, sqrt(dt), sqrt(1 - rho^2)):

    beta = 1    x += -sigma^2 dt / 2 + sigma sqrt(dt) Z1,  x = ln(F_t / F)
    beta < 1    G = F + sigma F^beta sqrt(dt) Z1;  F = G if F > 0 and G > 0, else 0 (absorbed)
    sigma *= exp(nu sqrt(dt) (rho Z1 + sqrt(1 - rho^2) Z2') - nu^2 dt / 2), after the F step

The mirror leg is the point -z.  Models, payoffs and levels are tests/sabr_oracle.py's.
"""
import math

import numpy as np

from tests import sabr_oracle as so
from tests.sabr_oracle import DOWN, F0, MODELS, R, T, UP, level_clearance, level_of, payoffs  # noqa: F401  (the GPU module's constants)
from tests.sobol_reference import bridge_walk, normal_chunks

LONG = so.LONG
SEED = 20240229
POINTS = (1, 65, 257, 4133)                    # one lane; a block and a lane; four waves and a lane; 17 workgroups with a ragged tail
STEPS = (1, 2, 13, 64, 65, 252, 1024)          # one node; a sweep batch of 4 cut short; 13; one whole fold of 64 dimensions; a fold plus; 252; the bridge's cap
SEQUENTIAL_ONLY = 1025                         # beyond the bridge's cap
CASES = [(name, POINTS[(i + j) % 4], n) for i, n in enumerate(STEPS + (SEQUENTIAL_ONLY,)) for j, name in enumerate(MODELS)]


def constructions(n):
    """bridge flags a shape is run with."""
    return (True, False) if n <= 1024 else (False,)


def normals(n, N, seed=SEED):
    """z (N, 2n) of points [0, N) of Sobol(d = 2n, scramble=True, seed)."""
    return np.concatenate(list(normal_chunks(2 * n, N, seed, 4096)))


def step_normals(z, bridge):
    """(Z1, Z2') of every step, each (N, n), from a point's 2n normals."""
    if not bridge:
        return z[:, 0::2], z[:, 1::2]
    return np.diff(bridge_walk(z[:, 0::2]), axis=1), np.diff(bridge_walk(z[:, 1::2]), axis=1)


def paths(F, T, model, n, z1, z2, mirror=False, dtype=LONG):
    """(forward, vol, closest): the matrices, each (count, n + 1), column 0 = (F, alpha) as given, and the smallest |G| any live path
    formed before the clamp (inf for beta = 1, which has none)."""
    alpha, beta, rho, nu = model
    dt = T / n
    sqrt_dt, rho_c = dtype(math.sqrt(dt)), dtype(math.sqrt(1 - rho * rho))
    sign = dtype(-1.0 if mirror else 1.0)
    z1 = sign * np.asarray(z1).astype(dtype)
    w = dtype(rho) * z1 + rho_c * (sign * np.asarray(z2).astype(dtype))
    count = z1.shape[0]
    forward, vol = np.empty((count, n + 1), dtype=dtype), np.empty((count, n + 1), dtype=dtype)
    forward[:, 0], vol[:, 0] = F, alpha
    f = np.full(count, F, dtype=dtype)
    x = np.zeros(count, dtype=dtype)
    sg = np.full(count, alpha, dtype=dtype)
    nu_l, half_dt = dtype(nu), dtype(0.5) * dtype(dt)
    closest = math.inf
    for t in range(n):
        if beta == 1.0:
            x = x - sg * sg * half_dt + sg * sqrt_dt * z1[:, t]
            f = dtype(F) * np.exp(x)
        else:
            live = f > 0
            safe = np.where(live, f, dtype(1))
            power = dtype(1) if beta == 0.0 else np.sqrt(safe) if beta == 0.5 else np.exp(dtype(beta) * np.log(safe))
            g = f + sg * power * sqrt_dt * z1[:, t]
            if live.any():
                closest = min(closest, float(np.min(np.abs(g[live]))))
            f = np.where(live & (g > 0), g, dtype(0))
        sg = sg * np.exp(nu_l * sqrt_dt * w[:, t] - nu_l * nu_l * half_dt)
        forward[:, t + 1], vol[:, t + 1] = f, sg
    return forward, vol, closest


BLACK_MODEL, BLACK_POINTS, BLACK_STEPS, BLACK_SIGMA = (0.25, 1.0, -0.4, 0.0), 1 << 14, 16, 0.25       # nu = 0, beta = 1: Black-76 at alpha


def black_case_price(is_call, K=100.0):
    """The oracle's discounted European price of the Black-76 case, on the bridge."""
    forward = case_paths(None, BLACK_POINTS, BLACK_STEPS, True, False, model=BLACK_MODEL)[0].astype(np.float64)
    return float(np.exp(-R * T) * np.mean(payoffs(forward, 8, is_call, K)))


def case_paths(name, N, n, bridge, mirror, z=None, model=None):
    """paths of a model of MODELS on points [0, N) (or on the points whose 2n normals are the rows of z)."""
    z1, z2 = step_normals(normals(n, N) if z is None else z, bridge)
    return paths(F0, T, MODELS[name] if model is None else model, n, z1, z2, mirror)
