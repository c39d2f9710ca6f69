"""Oracles of the Heston scenario tests (not a test module).

tests/heston_path_oracle.py's literal recursion (src/pricing_models/heston.py:291-303) and its inverse, with the scenario's own
(S, T, r, q) in place of that module's constants, and the Sobol step normals of that module -- which do not depend on T: a scenario
with another maturity reads the same (Z1, Z2') with its own dt.
"""
import numpy as np

from tests import heston_path_oracle as hpo
from tests.sobol_reference import normal_chunks


def literal_recursion(z1, z2p, model, n, S, T, r, q):
    """heston.py:291-303 with the given normals (each (m, n)): spot and variance, each (m, n + 1)."""
    kappa, theta, sigma_v, rho, v0 = model
    dt = T / n
    sqrt_dt = np.sqrt(dt)
    rho_sqrt = np.sqrt(1 - rho**2)
    m = z1.shape[0]
    spot, var = np.zeros((m, n + 1)), np.zeros((m, n + 1))
    spot[:, 0], var[:, 0] = S, v0
    log_S = np.log(S) * np.ones(m)
    v = v0 * np.ones(m)
    for t in range(1, n + 1):
        Z1 = z1[:, t - 1]
        Z2 = rho * Z1 + rho_sqrt * z2p[:, t - 1]
        v_pos = np.maximum(v, 0)
        sqrt_v = np.sqrt(v_pos)
        log_S += (r - q - 0.5 * v_pos) * dt + sqrt_v * sqrt_dt * Z1
        v += kappa * (theta - v_pos) * dt + sigma_v * sqrt_v * sqrt_dt * Z2
        v = np.maximum(v, 0)
        spot[:, t] = np.exp(log_S)
        var[:, t] = v
    return spot, var


def recovered_normals(spot, var, model, T, r, q):
    """(Z1, Z2') of every step from the states of a path whose variance never touched 0: the recursion solved for its normals."""
    kappa, theta, sigma_v, rho, _v0 = model
    n = spot.shape[1] - 1
    dt = T / n
    v = var[:, :-1]
    sd = np.sqrt(v * dt)
    z1 = (np.diff(np.log(spot), axis=1) - (r - q - 0.5 * v) * dt) / sd
    z2 = (np.diff(var, axis=1) - kappa * (theta - v) * dt) / (sigma_v * sd)
    return z1, (z2 - rho * z1) / np.sqrt(1 - rho**2)


def sobol_step_normals(n, n_points, seed, constructions, chunk=1024):
    """{construction: (Z1, Z2')}, each (n_points, n), of Sobol points [0, n_points): computed once and shared by every scenario."""
    parts = {c: ([], []) for c in constructions}
    for z in normal_chunks(2 * n, n_points, seed, chunk, None):
        for c in constructions:
            z1, z2p = hpo.step_normals(z, c)
            parts[c][0].append(z1)
            parts[c][1].append(z2p)
    return {c: (np.concatenate(a), np.concatenate(b)) for c, (a, b) in parts.items()}


def terminal_spots(normals, scenario, n, legs=(0,)):
    """The terminal spot of every path under the scenario (S, K, T, r, q, is_call, kappa, theta, sigma_v, rho, v0), the given legs
    concatenated (leg 1 is the mirror -z)."""
    z1, z2p = normals
    S, _K, T, r, q, _c, *model = scenario
    return np.concatenate([literal_recursion(sign * z1, sign * z2p, tuple(model), n, S, T, r, q)[0][:, -1]
                           for sign in [(1.0, -1.0)[leg] for leg in legs]])


def payoff(spot_T, scenario):
    return np.maximum((1.0 if scenario[5] else -1.0) * (spot_T - scenario[1]), 0)
