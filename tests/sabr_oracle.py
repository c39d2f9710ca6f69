"""The SABR path matrices as an extended-precision recursion on the stream's own draws (not a test module).

include/olmc_sabr.h restated from outside the device, in tests/path_draw_oracle.py's manner: the Philox words from the CPU oracle under
tag 0x53414252, the RAW normals from a Box-Muller tap (the instrumented build's on a GPU, tests/box_muller_reference.py without one),
block b feeding steps 2b and 2b + 1 as the Heston Euler stream does, and everything after them in np.longdouble on the constants the
host folds in fp64 (dt, sqrt(dt), sqrt(1 - rho^2)):

    beta = 1    ln F += -sigma^2 dt / 2 + sigma sqrt(dt) Z1
    beta < 1    G = F + sigma F^beta sqrt(dt) Z1;  F = G if F > 0 and G > 0, else 0 (absorbed)
    sigma *= exp(nu sqrt(dt) (rho Z1 + sqrt(1 - rho^2) Z2') - nu^2 dt / 2), after the F step

Payoffs: oracle/numpy_reference.py's restatements of the reference's Asian, barrier and lookback payoffs (the functions
tests/heston_path_oracle.payoffs applies), on the forward matrix, by the C ABI's payoff code.
"""
import math

import numpy as np

from oracle import numpy_reference as orc
from tests import path_draw_oracle as pdo

TAG_SABR = 0x53414252
LONG = pdo.LONG

F0, T, R = 100.0, 1.0, 0.03
SEED = (0x9E3779B9 << 32) | 20240229
PATHS = (100, 257, 4133)
STEPS = (1, 5, 13, 64)
UP, DOWN = 112.0, 90.0
# alpha beta rho nu
MODELS = {
    "lognormal": (0.25, 1.0, -0.4, 0.5),
    "half": (2.5, 0.5, -0.3, 0.4),
    "general": (0.9, 0.7, 0.2, 0.6),
    "normal-absorbing": (60.0, 0.0, -0.7, 0.8),
    "half-absorbing": (6.0, 0.5, -0.7, 1.0),
}
ABSORBING = ("normal-absorbing", "half-absorbing")
BARRIER_KINDS = ("up-and-out", "up-and-in", "down-and-out", "down-and-in")


def draws(seed, path_offset, count, n, box_muller):
    """(Z1, Z2') RAW of every step, each [count, n]."""
    blocks = (n + 1) // 2
    raw = pdo.draws(seed, path_offset, count, blocks, TAG_SABR, box_muller)[1]
    return raw[..., 0::2].reshape(count, 2 * blocks)[:, :n], raw[..., 1::2].reshape(count, 2 * blocks)[:, :n]


def paths(F, T, model, n, z1_raw, z2_raw, mirror=False, dtype=LONG):
    """(forward, vol, closest): the matrices, each (count, n + 1), column 0 = (F, alpha) as given, and the smallest |G| any live path
    formed before the clamp (inf for beta = 1, which has none)."""
    alpha, beta, rho, nu = model
    dt = T / n
    sqrt_dt, rho_c = dtype(math.sqrt(dt)), dtype(math.sqrt(1 - rho * rho))
    scale = -pdo.z_scale(dtype) if mirror else pdo.z_scale(dtype)
    z1 = scale * z1_raw.astype(dtype)
    w = dtype(rho) * z1 + rho_c * (scale * z2_raw.astype(dtype))
    count = z1.shape[0]
    forward, vol = np.empty((count, n + 1), dtype=dtype), np.empty((count, n + 1), dtype=dtype)
    forward[:, 0], vol[:, 0] = F, alpha
    f = np.full(count, F, dtype=dtype)
    lf = np.log(f)
    sg = np.full(count, alpha, dtype=dtype)
    nu_l, half_dt = dtype(nu), dtype(0.5) * dtype(dt)
    closest = math.inf
    for t in range(n):
        if beta == 1.0:
            lf = lf - sg * sg * half_dt + sg * sqrt_dt * z1[:, t]
            f = np.exp(lf)
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


def gbm_paths(F, T, sigma, n, z1_raw, dtype=LONG):
    """F exp(cumsum(-sigma^2 dt / 2 + sigma sqrt(dt) Z1)): what nu = 0, beta = 1 must reproduce."""
    dt = T / n
    z1 = pdo.z_scale(dtype) * z1_raw.astype(dtype)
    out = np.empty((z1.shape[0], n + 1), dtype=dtype)
    out[:, 0] = F
    out[:, 1:] = dtype(F) * np.exp(np.cumsum(dtype(sigma) * dtype(math.sqrt(dt)) * z1 - dtype(0.5 * sigma * sigma) * dtype(dt), axis=1))
    return out


def payoffs(forward, code, is_call, K, level=0.0):
    """The undiscounted payoff of every row of the forward matrix for the codes of olsb_price: 0-3 barriers, 4 / 5 floating / fixed
    lookback, 6 / 7 arithmetic / geometric Asian, 8 European."""
    forward = np.asarray(forward, dtype=np.float64)
    kind = "call" if is_call else "put"
    with np.errstate(divide="ignore"):                        # an absorbed path: ln 0 = -inf, a geometric mean of 0
        if code <= 3:
            return orc.barrier_from_paths(forward, K, T, R, level, BARRIER_KINDS[code], kind, return_payoffs=True)[1]
        if code <= 5:
            return orc.lookback_from_paths(forward, K, T, R, "floating" if code == 4 else "fixed", kind, return_payoffs=True)[1]
        if code <= 7:
            return orc.asian_from_paths(forward, K, T, R, "arithmetic" if code == 6 else "geometric", kind, return_payoffs=True)[1]
    return np.maximum((1.0 if is_call else -1.0) * (forward[:, -1] - K), 0.0)


def level_of(code):
    return UP if code <= 1 else DOWN if code <= 3 else 0.0


def level_clearance(forward):
    """The closest approach, in log space, of any positive state to a barrier level."""
    live = forward[forward > 0]
    return min(float(np.min(np.abs(np.log(live / UP)))), float(np.min(np.abs(np.log(live / DOWN)))))
