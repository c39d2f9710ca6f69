"""The three Philox path matrices as an extended-precision recursion on the stream's own draws (not a test module).

olmc_gbm_paths, olmc_heston_paths (Euler) and olmc_jump_paths / oljd_paths are what the suite's tight ties stand on: the payoffs NumPy
computes from them are the reference of the Heston, jump and exotic kernels.  Here each of them is restated from outside the device:

  words    oracle.philox_oracle.philox_words (integer-exact, any tag);
  normals  box_muller(x_a, x_b) -> (cosine, sine) in RAW fp32 units: the instrumented build's tap of the device's own box_muller_raw on
           a GPU, tests/box_muller_reference.py without one;
  uniforms unit_open64(x) = (x + 1/2) 2^-32, exact in fp64;
  the rest in np.longdouble (x86: 64 mantissa bits, 63 stored; WIDE says whether it is wider than fp64 here, and where it is not the
  recursions run in fp64 and the comparison of the two evaluations is empty), starting from the constants the HOST folds in fp64 (olmc.hip:
  gbm_step, make_heston, make_jump): dt, drift, vol = sigma sqrt(dt), mu_dt, kappa_dt, sqrt(dt), sqrt(1 - rho^2), lambda dt,
  p0 = exp(-lambda dt), kappa = E[e^Y - 1].  Python's float arithmetic is the host's.

The mapping of words to steps is the kernels' comments (olmc_kernels.h):

  GBM     block b, tag 0: the normals of steps 4b .. 4b + 3 are cos(x0, x1), sin(x0, x1), cos(x2, x3), sin(x2, x3);
  Heston  block b, tag 1: step 2b takes (Z1, Z2') = (cos, sin)(x0, x1), step 2b + 1 (cos, sin)(x2, x3);
  jump    block b, tag 2: (cos, sin)(x0, x1) are the diffusion normals of steps 2b and 2b + 1, x2 and x3 their Poisson uniforms;
          Merton's size normal of step t is cos(x0, x1) of block t, tag 3; Kou's jump j of step t takes (u_d, u_m) from words 2 (j % 2),
          2 (j % 2) + 1 of block t, tag 3 + j // 2.

These matrices add every normal in fp64.  The kernels that first sum a path's normals in fp32 chains (the European family, the cliquet's
period sums, the geometric Asian's prefix sums) are pinned in tests/normal_sum_oracle.py, which replays those chains bit for bit on the
same words and the same tap.

The cases of tests/test_gpu_path_matrices_exact.py are fixed here, so that tests/test_path_draw_oracle_cpu.py can hold the conditions
on their Poisson uniforms (no uniform within 1e-12 of a step of the CDF, no count at the cap of 64) without a device.
"""
import functools
import math

import numpy as np

from oracle import philox_oracle
from tests import heston_path_oracle as hpo

TAG_GBM, TAG_HESTON, TAG_JUMP, TAG_JUMP_SIZE = 0, 1, 2, 3
JUMP_CAP = 64
WIDE = bool(np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant)
LONG = np.longdouble if WIDE else np.float64


def z_scale(dtype=LONG):
    """sqrt(2 ln 2) in dtype: a true normal is this times a RAW one (kZScale is its fp64 rounding)."""
    return np.sqrt(dtype(2) * np.log(dtype(2)))


# ------------------------------------------------------------------------------------------------------------ draws ----
_WORDS = {}


def philox_words(seed, path_offset, count, blocks, tag):
    """philox_oracle.philox_words(seed, path_offset, count, 0, blocks, tag), kept: a later call for more blocks draws only the new ones."""
    key = (int(seed), int(path_offset), int(count), int(tag))
    have = _WORDS.get(key)
    if have is None or have.shape[1] < blocks:
        first = 0 if have is None else have.shape[1]
        more = philox_oracle.philox_words(seed, path_offset, count, first, blocks - first, tag)
        have = more if have is None else np.concatenate([have, more], axis=1)
        _WORDS[key] = have
    return have[:, :blocks]


def unit_open64(x):
    return (np.asarray(x).astype(np.float64) + 0.5) * 2.0**-32


def raw_pair(box_muller, xa, xb):
    """(cosine, sine) of the tap as fp64 values of its fp32 results, in the words' shape."""
    xa, xb = np.asarray(xa, dtype=np.uint32), np.asarray(xb, dtype=np.uint32)
    if xa.size == 0:
        return np.zeros(xa.shape), np.zeros(xa.shape)
    z_cos, z_sin = box_muller(xa.ravel(), xb.ravel())[:2]
    return (np.asarray(z_cos, dtype=np.float32).astype(np.float64).reshape(xa.shape),
            np.asarray(z_sin, dtype=np.float32).astype(np.float64).reshape(xa.shape))


def draws(seed, path_offset, count, blocks, tag, box_muller):
    """(words, raw, unit), each [count, blocks, 4]: the Philox words of paths [path_offset, path_offset + count), the RAW normals
    (cos, sin)(x0, x1), (cos, sin)(x2, x3) in that order, and unit_open64 of every word."""
    words = philox_words(seed, path_offset, count, blocks, tag)
    c0, s0 = raw_pair(box_muller, words[..., 0], words[..., 1])
    c1, s1 = raw_pair(box_muller, words[..., 2], words[..., 3])
    return words, np.stack([c0, s0, c1, s1], axis=-1), unit_open64(words)


def reference_box_muller(xa, xb):
    """The tap's stand-in without a device: tests/box_muller_reference.py's fp64 transform, rounded to fp32."""
    from tests import box_muller_reference as bm

    _rad, z_cos, z_sin, _pair = bm.raw(xa, xb)
    return z_cos.astype(np.float32), z_sin.astype(np.float32)


def gbm_draws(seed, path_offset, count, n, box_muller):
    """The RAW normal of every step, [count, n]."""
    blocks = (n + 3) // 4
    raw = draws(seed, path_offset, count, blocks, TAG_GBM, box_muller)[1]
    return raw.reshape(count, 4 * blocks)[:, :n]


def heston_draws(seed, path_offset, count, n, box_muller):
    """(Z1, Z2') RAW of every step, each [count, n]."""
    blocks = (n + 1) // 2
    raw = draws(seed, path_offset, count, blocks, TAG_HESTON, box_muller)[1]
    return raw[..., 0::2].reshape(count, 2 * blocks)[:, :n], raw[..., 1::2].reshape(count, 2 * blocks)[:, :n]


def jump_draws(seed, path_offset, count, n, box_muller):
    """(z, u): the RAW diffusion normal and the Poisson uniform of every step, each [count, n]."""
    blocks = (n + 1) // 2
    _words, raw, unit = draws(seed, path_offset, count, blocks, TAG_JUMP, box_muller)
    return raw[..., 0:2].reshape(count, 2 * blocks)[:, :n], unit[..., 2:4].reshape(count, 2 * blocks)[:, :n]


def poisson_uniforms(seed, path_offset, count, n):
    """jump_draws' u alone: it needs no normals, so no tap."""
    blocks = (n + 1) // 2
    return unit_open64(philox_words(seed, path_offset, count, blocks, TAG_JUMP)[..., 2:4]).reshape(count, 2 * blocks)[:, :n]


@functools.lru_cache(maxsize=None)
def _size_block(seed, path, step, tag):
    return philox_oracle.philox_words(seed, path, 1, step, 1, tag)[0, 0]


def size_words(seed, paths, steps, tag):
    """words[k, 4] of block (paths[k], steps[k], tag): drawn one by one, only where a path jumps."""
    out = np.empty((len(paths), 4), dtype=np.uint32)
    for k, (p, t) in enumerate(zip(paths, steps)):
        out[k] = _size_block(int(seed), int(p), int(t), int(tag))
    return out


# ------------------------------------------------------------------------------------------------------------- GBM ----
def gbm_constants(S, T, r, sigma, q, n):
    dt = T / n
    return dict(log_s0=math.log(S), drift=(r - q - 0.5 * sigma * sigma) * dt, vol=sigma * math.sqrt(dt))


def gbm_cum(c, z_raw, dtype=LONG):
    """cum[count, n]: the cumulative log-return after every step, cum += vol kZScale z + drift."""
    return np.cumsum(dtype(c["vol"]) * z_scale(dtype) * z_raw.astype(dtype) + dtype(c["drift"]), axis=1)


def gbm_paths(S, T, r, sigma, q, n, z_raw, dtype=LONG):
    """(count, n + 1) spots, column 0 = S."""
    c = gbm_constants(S, T, r, sigma, q, n)
    out = np.empty((z_raw.shape[0], n + 1), dtype=dtype)
    out[:, 0] = S
    out[:, 1:] = np.exp(dtype(c["log_s0"]) + gbm_cum(c, z_raw, dtype))
    return out


def gbm_bound(cum):
    """[count, n]: the bound on |ln S_device - ln S_reference| at dates 1 .. n, (t + 8) M 2^-52 with M = max(1, max_t |cum|) of the path.

    The device rounds cum twice per step (the fma of the increment, at most 2^-53 |increment|, and the addition, at most 2^-53 |cum|:
    together under M 2^-52 a step), ln S + cum once ((ln 100 + M) 2^-53 < 2.8 M 2^-52), its exponential is within one ulp (2^-52 of
    ln S), and vol kZScale carries kZScale's own rounding and the product's (2^-52 relative on the normals' part of cum, under
    M 2^-52): t + 4.8 of these units, rounded up to t + 8."""
    m = np.maximum(1.0, np.max(np.abs(cum.astype(np.float64)), axis=1, keepdims=True))
    t = np.arange(1, cum.shape[1] + 1, dtype=np.float64)
    return (t + 8.0) * m * 2.0**-52


# ---------------------------------------------------------------------------------------------------------- Heston ----
def heston_paths(S, model, T, r, q, n, z1_raw, z2_raw, mirror=False, dtype=LONG):
    """(spot, var), each (count, n + 1), column 0 = (S, v0) as given: the literal recursion of heston_path_oracle.literal_recursion
    (heston.py:291-303) on the RAW normals, with v+ = max(v, 0) entering the step (so v0 < 0 makes the first step deterministic, as
    heston_start has it) and the truncation at 0 after it.  The mirror leg takes -Z1, -Z2'."""
    kappa, theta, sigma_v, rho, v0 = model
    dt = T / n
    mu_dt, kappa_dt, sqrt_dt, rho_c = dtype((r - q) * dt), dtype(kappa * dt), dtype(math.sqrt(dt)), dtype(math.sqrt(1 - rho * rho))
    scale = (-z_scale(dtype) if mirror else z_scale(dtype))
    z1 = scale * z1_raw.astype(dtype)
    z2 = dtype(rho) * z1 + rho_c * (scale * z2_raw.astype(dtype))
    count = z1.shape[0]
    spot, var = np.empty((count, n + 1), dtype=dtype), np.empty((count, n + 1), dtype=dtype)
    spot[:, 0], var[:, 0] = S, v0
    ls = np.full(count, math.log(S), dtype=dtype)
    v = np.full(count, v0, dtype=dtype)
    half_dt, theta, sigma_v = dtype(0.5) * dtype(dt), dtype(theta), dtype(sigma_v)
    for t in range(n):
        v_pos = np.maximum(v, 0)
        root = np.sqrt(v_pos)
        ls = ls + (mu_dt - half_dt * v_pos) + root * sqrt_dt * z1[:, t]
        v = np.maximum(v + kappa_dt * (theta - v_pos) + sigma_v * root * sqrt_dt * z2[:, t], 0)
        spot[:, t + 1] = np.exp(ls)
        var[:, t + 1] = v
    return spot, var


# ------------------------------------------------------------------------------------------------------------ jump ----
def jump_kappa(model):
    """E[e^Y - 1] as make_jump forms it (jump_diffusion.py:64-67 Merton, :293-299 Kou)."""
    kou, _lam, a1, a2, a3 = model
    return (a1 * a2 / (a2 - 1) + (1 - a1) * a3 / (a3 + 1) - 1) if kou else math.exp(a1 + 0.5 * a2 * a2) - 1


def jump_constants(S, T, r, sigma, q, model, n):
    _kou, lam, _a1, _a2, _a3 = model
    dt = T / n
    lam_dt = lam * dt
    return dict(log_s0=math.log(S), dt=dt, drift=(r - q - lam * jump_kappa(model) - 0.5 * sigma * sigma) * dt, vol=sigma * math.sqrt(dt),
                lam_dt=lam_dt, p0=math.exp(-lam_dt))


def poisson_cdf_steps(p0, lam_dt, dtype=LONG):
    """CDF(0) .. CDF(64) by the kernel's recurrence pk *= lam_dt / k."""
    pk = dtype(p0)
    out = [pk]
    for k in range(1, JUMP_CAP + 1):
        pk = pk * (dtype(lam_dt) / dtype(k))
        out.append(out[-1] + pk)
    return np.array(out, dtype=dtype)


def counts_by_the_loop(u, p0, lam_dt, dtype=LONG):
    """The kernel's inversion (jump_sizes): 0 if u < p0, else the first n <= 64 with u < CDF(n)."""
    cdf = poisson_cdf_steps(p0, lam_dt, dtype)
    u = np.asarray(u).astype(dtype)
    n = np.zeros(u.shape, dtype=np.int64)
    for k in range(JUMP_CAP):
        n += u >= cdf[k]                                                           # the CDF rises: u >= CDF(k) implies u >= CDF(k - 1)
    return n


def counts_by_ppf(u, lam_dt):
    """The same count with nothing of the kernel in it: SciPy's quantile of Poisson(lambda dt)."""
    from scipy.stats import poisson

    if lam_dt == 0.0:
        return np.zeros(np.shape(u), dtype=np.int64)
    return poisson.ppf(u, lam_dt).astype(np.int64)


def distance_to_a_cdf_step(u, lam_dt):
    """min over u and k <= 64 of |u - CDF(k)| (SciPy's CDF): a uniform this close to a step may be counted either way."""
    from scipy.stats import poisson

    if lam_dt == 0.0:
        return float(np.min(1.0 - np.asarray(u)))
    cdf = poisson.cdf(np.arange(JUMP_CAP + 1), lam_dt)
    cdf = cdf[cdf < 1.0]
    return float(np.min(np.abs(np.asarray(u)[..., None] - cdf)))


def jump_sums(seed, path_offset, model, counts, box_muller, dtype=LONG):
    """[count, n]: the sum of the jump sizes of every step.  Merton: n mu_j + sigma_j sqrt(n) z.  Kou: the terms in jump order,
    -log(u_m) / eta1 if u_d < p, else log(u_m) / eta2."""
    kou, _lam, a1, a2, a3 = model
    out = np.zeros(counts.shape, dtype=dtype)
    paths, steps = np.nonzero(counts)
    if paths.size == 0:
        return out
    k = counts[paths, steps]
    if not kou:
        w = size_words(seed, path_offset + paths, steps, TAG_JUMP_SIZE)
        z = z_scale(dtype) * raw_pair(box_muller, w[:, 0], w[:, 1])[0].astype(dtype)
        out[paths, steps] = k.astype(dtype) * dtype(a1) + dtype(a2) * np.sqrt(k.astype(dtype)) * z
        return out
    for j in range(int(k.max())):
        live = k > j
        w = size_words(seed, path_offset + paths[live], steps[live], TAG_JUMP_SIZE + j // 2)
        u_d, u_m = unit_open64(w[:, 2 * (j % 2)]), unit_open64(w[:, 2 * (j % 2) + 1]).astype(dtype)
        out[paths[live], steps[live]] += np.where(u_d < a1, -np.log(u_m) / dtype(a2), np.log(u_m) / dtype(a3))
    return out


def jump_paths(S, T, r, sigma, q, model, n, z_raw, sums, mirror=False, dtype=LONG):
    """(count, n + 1) spots, column 0 = S: ls += vol kZScale z + drift, then the step's jump sum; the mirror takes -z on the same jumps."""
    c = jump_constants(S, T, r, sigma, q, model, n)
    vol = (-1 if mirror else 1) * dtype(c["vol"]) * z_scale(dtype)
    ls = dtype(c["log_s0"]) + np.cumsum((vol * z_raw.astype(dtype) + dtype(c["drift"])) + sums.astype(dtype), axis=1)
    out = np.empty((z_raw.shape[0], n + 1), dtype=dtype)
    out[:, 0] = S
    out[:, 1:] = np.exp(ls)
    return out


def jump_oracle(S, T, r, sigma, q, model, n, seed, path_offset, count, box_muller, dtype=LONG):
    """dict(plain, mirror: spots (count, n + 1); counts, sums: [count, n]; u) of paths [path_offset, path_offset + count)."""
    c = jump_constants(S, T, r, sigma, q, model, n)
    z_raw, u = jump_draws(seed, path_offset, count, n, box_muller)
    counts = counts_by_the_loop(u, c["p0"], c["lam_dt"], dtype)
    sums = jump_sums(seed, path_offset, model, counts, box_muller, dtype)
    return dict(u=u, counts=counts, sums=sums, plain=jump_paths(S, T, r, sigma, q, model, n, z_raw, sums, False, dtype),
                mirror=jump_paths(S, T, r, sigma, q, model, n, z_raw, sums, True, dtype))


# ------------------------------------------------------------------------------- the cases of the GPU module ----
S, T, R, Q = hpo.S, hpo.T, hpo.R, hpo.Q
SIGMA = 0.2
BIG_SEED = (0x9E3779B9 << 32) | 20240229
SMALL_SEED = 3
STEPS = (1, 2, 3, 4, 5, 7, 13, 64, 252)                    # every remainder of the 4-step and of the 2-step blocks
# N: one path, less than a wave, one past a workgroup, 17 workgroups with a ragged last one.  The oracle's words cost 25 us a block, so
# the longest grids go with the fewest paths: every n at N = 1 and 63, n <= 64 at 257, n <= 7 at 4133.
STEPS_OF = {1: STEPS, 63: STEPS, 257: STEPS[:-1], 4133: STEPS[:6]}
SMALL_SEED_SHAPES = ((1, 5), (63, 13), (257, 7), (4133, 2))


def shapes(N):
    """(seed, n) of the launches of N paths."""
    return [(BIG_SEED, n) for n in STEPS_OF[N]] + [(SMALL_SEED, n) for count, n in SMALL_SEED_SHAPES if count == N]


# (sigma, T, r, q): q > r, a volatile two-year grid, no volatility at all
GBM_PARAMS = ((0.2, 1.0, 0.01, 0.05), (1.5, 2.0, 0.01, 0.05), (0.0, 1.0, 0.01, 0.05))

# kappa theta sigma_v rho v0
HESTON_MODELS = {"usual": hpo.USUAL, "feller_violating": hpo.FELLER_VIOLATING, "v0_zero": (*hpo.USUAL[:4], 0.0),
                 "v0_negative": (*hpo.USUAL[:4], -0.002), "rho_zero": (*hpo.USUAL[:3], 0.0, hpo.USUAL[4]),
                 "rho_minus_one": (*hpo.USUAL[:3], -1.0, hpo.USUAL[4]), "sigma_v_zero": (*hpo.USUAL[:2], 0.0, *hpo.USUAL[3:])}

# (kou, lambda_j, a1, a2, a3): the four of tests/test_gpu_jump_payoffs.py, no jumps at all, and lambda dt = 20 exactly -- the last rate
# that is not refused -- as Merton at the n whose 20 n (T / n) is 20 in fp64, as Kou through K1 at n = 3 (60 (1 / 3) rounds to 20)
M0, M1, K0, K1 = (False, 0.5, -0.1, 0.2, 0.0), (False, 40.0, 0.02, 0.1, 0.0), (True, 1.0, 0.4, 10.0, 5.0), (True, 60.0, 0.6, 25.0, 20.0)
NO_JUMPS = (False, 0.0, -0.1, 0.2, 0.0)


def merton_20(n):
    return (False, 20.0 * n, 0.02, 0.1, 0.0)


def refused(model, n):
    """More than 20 expected jumps per step, by the host's own product."""
    return model[1] * (T / n) > 20.0


def jump_cases(N):
    """(name, model, seed, n) of the launches of N paths.  The size blocks are drawn one by one, so the intense models take the
    shorter grids as N grows: a step of K1 at lambda dt = 20 reads about ten blocks."""
    out = []
    for seed, n in shapes(N):
        for name, model in (("M0", M0), ("K0", K0), ("no_jumps", NO_JUMPS)):
            out.append((name, model, seed, n))
        if not refused(M1, n) and (N <= 257 or n == 2):
            out.append(("M1", M1, seed, n))
        if not refused(K1, n) and (N <= 63 or (N == 257 and n == 3)):
            out.append(("K1", K1, seed, n))
    for count, n in ((1, 1), (1, 2), (1, 4), (1, 64), (63, 4), (257, 2), (4133, 1)):
        if count == N:
            out.append(("merton_20", merton_20(n), BIG_SEED, n))
    return out


OFFSETS = ((1 << 32) - 1, (1 << 32) + 5, (1 << 40) + 3)
OFFSET_STEPS = (1, 2, 3, 4, 13)
