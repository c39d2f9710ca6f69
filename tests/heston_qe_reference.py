"""NumPy restatement of Heston's quadratic-exponential step and of a path (not a test module).

Written from the formulas of include/olmc.h ("Heston, quadratic-exponential scheme") in the folded constants the host computes
(olmc.hip: make_heston_qe): E, 1 - E through expm1, the two coefficients of s^2, K1, K2, K3 = K4 and (r - q) dt + K0 as ONE per-date
drift.  It is fed the draws as matrices (u_v, z_v, z_s), each (paths, steps): where they come from -- SciPy's Sobol points, the Philox
oracle's words -- is the caller's business (sobol_draws, philox_draws below).  The mirror leg is the same recursion on
(1 - u_v, -z_v, -z_s).
"""
import math

import numpy as np

PSI_C = 1.5
STREAM_HESTON_QE = 0x48514500                                # OLMC_STREAM_HESTON_QE

# kappa theta sigma_v rho v0
FELLER_VIOLATED = (1.0, 0.09, 1.0, -0.3, 0.09)               # 2 kappa theta = 0.18 < sigma_v^2 = 1: both branches
STEEP = (0.5, 0.04, 1.0, -0.9, 0.04)                         # both branches, rho = -0.9
USUAL = (2.0, 0.04, 0.3, -0.7, 0.04)                         # psi <= 0.5625 everywhere: the quadratic branch only
MODELS = {"feller_violated": FELLER_VIOLATED, "steep": STEEP, "usual": USUAL}


def constants(model, r, q, T, n):
    """The launch constants of n steps to T, folded as the host folds them."""
    kappa, theta, sigma_v, rho, _v0 = model
    dt = T / n
    e = math.exp(-kappa * dt)
    one_minus_e = -math.expm1(-kappa * dt)
    g = 0.5 * dt * (kappa * rho / sigma_v - 0.5)
    return dict(dt=dt, e=e, theta_1me=theta * one_minus_e,
                c1=sigma_v * sigma_v * e * one_minus_e / kappa,
                c2=theta * sigma_v * sigma_v * one_minus_e * one_minus_e / (2.0 * kappa),
                drift_dt=(r - q) * dt + -rho * kappa * theta * dt / sigma_v,
                k1=g - rho / sigma_v, k2=g + rho / sigma_v, k3=0.5 * dt * (1.0 - rho * rho))


def moments(v, c):
    """(m, s^2, psi) of the next variance given v >= 0."""
    v = np.asarray(v, dtype=np.float64)
    m = v * c["e"] + c["theta_1me"]
    s2 = v * c["c1"] + c["c2"]
    return m, s2, s2 / (m * m)


def exponential_p(v, c):
    """p of the exponential branch, (psi - 1) / (psi + 1) as (s^2 - m^2) / (s^2 + m^2)."""
    m, s2, _psi = moments(v, c)
    return (s2 - m * m) / (s2 + m * m)


def next_variance(v, u_v, z_v, c):
    """(v', quadratic) elementwise: the quadratic branch reads z_v, the exponential one u_v."""
    m, s2, _psi = moments(v, c)
    m2 = m * m
    quadratic = s2 <= PSI_C * m2
    with np.errstate(invalid="ignore", divide="ignore"):
        x = 2.0 * m2 / s2                                                         # 2 / psi
        b2 = (x - 1.0) + np.sqrt(x * np.maximum(x - 1.0, 0.0))
        a = m / (1.0 + b2)
        w = np.sqrt(b2) + z_v
        v_quadratic = a * (w * w)
        p = (s2 - m2) / (s2 + m2)
        beta = (1.0 - p) / m
        u = np.minimum(u_v, np.nextafter(1.0, 0.0))                               # only to keep the unused side finite
        v_exponential = np.where(u_v <= p, 0.0, np.log((1.0 - p) / (1.0 - u)) / beta)
    return np.where(quadratic, v_quadratic, v_exponential), quadratic


def paths(S, model, r, q, T, n, u_v, z_v, z_s, mirror=False):
    """spot, var: (paths, n + 1), column 0 = (S, v0) as given; quadratic: (paths, n) bool, the branch of every step; psi likewise."""
    c = constants(model, r, q, T, n)
    if mirror:
        u_v, z_v, z_s = 1.0 - u_v, -z_v, -z_s
    count = u_v.shape[0]
    spot, var = np.empty((count, n + 1)), np.empty((count, n + 1))
    quadratic, psi = np.empty((count, n), dtype=bool), np.empty((count, n))
    spot[:, 0], var[:, 0] = S, model[4]
    ls = np.full(count, math.log(S))                                              # without the drift: added per date
    v = np.full(count, float(model[4]))
    for t in range(n):
        psi[:, t] = moments(v, c)[2]
        vn, quadratic[:, t] = next_variance(v, u_v[:, t], z_v[:, t], c)
        ls = ls + c["k1"] * v + c["k2"] * vn + np.sqrt(c["k3"] * (v + vn)) * z_s[:, t]
        v = vn
        spot[:, t + 1] = np.exp(ls + (t + 1) * c["drift_dt"])
        var[:, t + 1] = v
    return spot, var, quadratic, psi


def sobol_draws(n, count, seed, first=0):
    """(u_v, z_v, z_s) of Sobol points [first, first + count): SciPy's Sobol(d=2n, scramble=True, seed), clipped to [1e-10, 1 - 1e-10];
    dimension 2t is U_v and Z_v = norm.ppf of it, dimension 2t + 1 gives Z_s."""
    from scipy.stats import norm, qmc

    engine = qmc.Sobol(d=2 * n, scramble=True, seed=seed)
    if first:
        engine.fast_forward(first)
    u = np.clip(engine.random(count), 1e-10, 1 - 1e-10)
    return u[:, 0::2], norm.ppf(u[:, 0::2]), norm.ppf(u[:, 1::2])


def philox_draws(words, box_muller):
    """(u_v, z_v, z_s) from the Philox blocks words[path, step, 4] of counter (path_lo, path_hi, step, STREAM_HESTON_QE):
    box_muller(x0, x1) -> (cosine, sine) in RAW fp32 units (the instrumented build's tap), scaled by sqrt(2 ln 2); U_v = (x2 + 1/2) 2^-32."""
    shape = words.shape[:2]
    z_cos, z_sin = box_muller(words[..., 0], words[..., 1])[:2]
    scale = math.sqrt(2.0 * math.log(2.0))
    z_v = scale * np.asarray(z_cos, dtype=np.float64).reshape(shape)
    z_s = scale * np.asarray(z_sin, dtype=np.float64).reshape(shape)
    u_v = (words[..., 2].astype(np.float64) + 0.5) * 2.0**-32
    return u_v, z_v, z_s


def heston_call(S, K, T, r, q, model):
    """The European call from the published P1 / P2 form of the characteristic function (Heston 1993, in the formulation of Albrecher et
    al. 2007 that stays on the principal branch), by quadrature."""
    from scipy.integrate import quad

    kappa, theta, sigma_v, rho, v0 = model
    x = math.log(S)

    def cf(phi, j):
        u = 0.5 if j == 1 else -0.5
        b = kappa - rho * sigma_v if j == 1 else kappa
        d = np.sqrt((rho * sigma_v * 1j * phi - b) ** 2 - sigma_v**2 * (2 * u * 1j * phi - phi * phi))
        g = (b - rho * sigma_v * 1j * phi - d) / (b - rho * sigma_v * 1j * phi + d)
        big_c = (r - q) * 1j * phi * T + kappa * theta / sigma_v**2 * ((b - rho * sigma_v * 1j * phi - d) * T
                                                                      - 2 * np.log((1 - g * np.exp(-d * T)) / (1 - g)))
        big_d = (b - rho * sigma_v * 1j * phi - d) / sigma_v**2 * (1 - np.exp(-d * T)) / (1 - g * np.exp(-d * T))
        return np.exp(big_c + big_d * v0 + 1j * phi * x)

    def prob(j):
        integrand = lambda phi: (np.exp(-1j * phi * math.log(K)) * cf(phi, j) / (1j * phi)).real
        return 0.5 + quad(integrand, 1e-12, 200.0, limit=400)[0] / math.pi

    return S * math.exp(-q * T) * prob(1) - K * math.exp(-r * T) * prob(2)
