"""NumPy restatement of the folded definition of include/olmc_jump_scenarios.h, independent of the device code.

A scenario is _hip's tuple (S, K, T, r, sigma, q, is_call, kou, lambda_j, a1, a2, a3).  For paths [path0, path0 + N) of a seed:
    Z     the sum over the steps, in step order, in fp64, of the path's raw Box-Muller normals (block (path, t / 2, tag 2), words 0, 1);
    J_g   the sum of the size terms of jump group g, steps ascending and, for Kou, jumps ascending; the count of a step by inversion of
          the step's one Poisson uniform (word 2 + t % 2) against the group's p0 = exp(-lambda T / n), at most 64;
    x_i   fma(vol_i, +-Z, n drift_i) + J_g(i);    payoff max(+-(exp(ln S_i + x_i) - K_i), 0); the mirror leg takes -Z and the same J.
Philox, the uniforms and the raw Box-Muller pair restate oracle/philox_gbm.c in vectorised NumPy (checked against it word for word in
tests/test_jump_scenarios_cpu.py).  fma(a, b, c) is formed as a * b + c in np.longdouble and rounded once: on x86-64 its 64-bit
significand holds the product's leading bits, and the double rounding differs from a true fma on a vanishing share of paths by one ulp
of x, far below the tests' bar.
"""
import math

import numpy as np

from oracle import philox_oracle as po  # noqa: F401  (re-exported: the tests compare against its jump_paths)

Z_SCALE = 1.1774100225154747          # sqrt(2 ln 2): the unit of a raw normal
TAG_JUMP, TAG_SIZE = 2, 3
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox(paths, block, tag, seed):
    """Words (4, len(paths)) of Philox4x32-10 at counter (path lo, path hi, block, tag) under the key of seed; block may be an array."""
    paths = np.asarray(paths, dtype=np.uint64)
    c0, c1 = paths & _MASK, paths >> np.uint64(32)
    c2 = np.broadcast_to(np.asarray(block, dtype=np.uint64), paths.shape).copy()
    c3 = np.broadcast_to(np.asarray(tag, dtype=np.uint64), paths.shape).copy()
    seed = int(seed) & ((1 << 64) - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & _MASK, p0 & _MASK, n0, n2
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def unit_open64(x):
    return (x.astype(np.float64) + 0.5) * 2.0**-32


def box_muller_raw(xa, xb):
    """The raw pair (cosine, sine) of philox_gbm.c: evaluated in double on the fp32 radius input, rounded once to fp32."""
    ua = (xa.astype(np.float32) * np.float32(2.0**-32) + np.float32(2.0**-33)).astype(np.float64)       # the product is exact: one rounding, as fmaf
    ub = (xb & np.uint32(0x007FFFFF)).astype(np.float64) * 2.0**-23
    rad, ang = np.sqrt(-np.log2(ua)), 6.283185307179586476925 * ub
    return (rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32)


def group_key(sc):
    kou, lam, a1, a2, a3 = sc[7:]
    return (bool(kou), np.float64(lam).tobytes(), np.float64(sc[2]).tobytes(), np.float64(a1).tobytes(), np.float64(a2).tobytes(),
            np.float64(a3).tobytes() if kou else b"")


def layout(scenarios):
    """(n_groups, group[k]): groups numbered by first appearance."""
    seen, group = [], []
    for sc in scenarios:
        key = group_key(sc)
        if key not in seen:
            seen.append(key)
        group.append(seen.index(key))
    return len(seen), group


def counts(u, lam_dt):
    """The jump count of a step by jump_sizes' inversion."""
    p0 = math.exp(-lam_dt)
    n = np.where(u < p0, 0, 1).astype(np.int32)
    pk = np.full(u.shape, p0 * lam_dt)
    cdf = p0 + pk
    for _ in range(63):
        more = (n >= 1) & (u >= cdf) & (n < 64)
        if not more.any():
            break
        n = np.where(more, n + 1, n)
        pk = np.where(more, pk * (lam_dt / np.maximum(n, 1)), pk)
        cdf = np.where(more, cdf + pk, cdf)
    return n


def walk(scenarios, N, n, seed, path0=0):
    """(Z[N], J[n_groups][N], group[k]) of the paths."""
    paths = np.arange(path0, path0 + N, dtype=np.uint64)
    n_groups, group = layout(scenarios)
    first = [group.index(g) for g in range(n_groups)]
    Z, J = np.zeros(N), [np.zeros(N) for _ in range(n_groups)]
    for t in range(n):
        w = philox(paths, t >> 1, TAG_JUMP, seed)
        zc, zs = box_muller_raw(w[0], w[1])
        Z = Z + (zs if t & 1 else zc).astype(np.float64)
        u = unit_open64(w[3] if t & 1 else w[2])
        size_words = {}

        def size_block(b):
            if b not in size_words:
                size_words[b] = philox(paths, t, TAG_SIZE + b, seed)
            return size_words[b]

        for g in range(n_groups):
            sc = scenarios[first[g]]
            kou, lam, a1, a2, a3 = sc[7:]
            cnt = counts(u, lam * (sc[2] / n))
            if not cnt.any():
                continue
            if not kou:
                k = size_block(0)
                z_jump = Z_SCALE * box_muller_raw(k[0], k[1])[0].astype(np.float64)
                term = cnt * a1 + a2 * np.sqrt(cnt.astype(np.float64)) * z_jump
                J[g] = np.where(cnt > 0, J[g] + term, J[g])
            else:
                inv1, inv2 = 1.0 / a2, 1.0 / a3
                for j in range(int(cnt.max())):
                    k = size_block(j >> 1)
                    ud, um = unit_open64(k[2] if j & 1 else k[0]), unit_open64(k[3] if j & 1 else k[1])
                    term = np.where(ud < a1, -np.log(um) * inv1, np.log(um) * inv2)
                    J[g] = np.where(cnt > j, J[g] + term, J[g])
    return Z, J, group


def kappa(sc):
    kou, _lam, a1, a2, a3 = sc[7:]
    return a1 * a2 / (a2 - 1) + (1 - a1) * a3 / (a3 + 1) - 1 if kou else math.exp(a1 + 0.5 * a2 * a2) - 1


def _fma(a, b, c):
    return (np.longdouble(a) * b.astype(np.longdouble) + np.longdouble(c)).astype(np.float64)


def payoffs(scenarios, N, n, seed, antithetic=False, path0=0):
    """[the payoffs of scenario i: N of them, or with antithetic the N of the path then the N of its mirror leg]."""
    Z, J, group = walk(scenarios, N, n, seed, path0)
    out = []
    for sc, g in zip(scenarios, group):
        S, K, T, r, sigma, q, call = sc[:7]
        dt = T / n
        drift = (r - q - sc[8] * kappa(sc) - 0.5 * sigma * sigma) * dt
        vol = sigma * math.sqrt(dt) * Z_SCALE
        sign = 1.0 if call else -1.0
        legs = []
        for mirror in ((False, True) if antithetic else (False,)):
            x = _fma(vol, -Z if mirror else Z, float(n) * drift) + J[g]
            legs.append(np.maximum(sign * (np.exp(math.log(S) + x) - K), 0.0))
        out.append(np.concatenate(legs))
    return out


def payoff(spot_last, sc):
    """The payoff of scenario sc on the last column of a path matrix."""
    return np.maximum((1.0 if sc[6] else -1.0) * (spot_last - sc[1]), 0.0)
