"""A plain restatement of the scrambled-Sobol points the device expands, and what the path oracles share (not a test module).

Point k of scipy.stats.qmc.Sobol(d, scramble=True, seed), as an integer: x_t(k) = shift[t] ^ XOR over the set bits b of gray(k) =
k ^ (k >> 1) of sv[t][b], 30 bits, k < 2^30.  Everything here is Python or uint64 integers and fp64; nothing follows the device
code's structure (no lane masks, no folds, no blocks of eight).  tests/test_sobol_reference_cpu.py pins it to SciPy's own engine,
the GPU tests then use it where SciPy's fast_forward (linear in offset x d) would take minutes.
"""
import collections
import math
import warnings

import numpy as np

BITS = 30
CLIP = 1e-10                       # src/simulation/gbm_qmc.py:36


def points(sv, shift, ks):
    """x[i][t] of the points ks (any integers below 2^30), uint64 (len(ks), d): the 30-step masked XOR over the Gray code."""
    sv = np.asarray(sv, dtype=np.uint64)
    ks = np.asarray(ks, dtype=np.uint64).reshape(-1)
    if sv.ndim != 2 or sv.shape[1] != BITS:
        raise ValueError("sv must be (d, 30)")
    if ks.size and int(ks.max()) >> BITS:
        raise ValueError("point index beyond 2^30")
    gray = ks ^ (ks >> np.uint64(1))
    x = np.repeat(np.asarray(shift, dtype=np.uint64)[:, None], ks.size, axis=1)          # (d, points): long rows are quicker to walk
    term = np.empty_like(x)
    for b in range(BITS):
        chosen = (gray >> np.uint64(b)) & np.uint64(1)
        np.multiply(sv[:, b, None], chosen[None, :], out=term)
        x ^= term
    return np.ascontiguousarray(x.T)


def uniforms(x):
    return np.asarray(x, dtype=np.float64) * 2.0 ** -BITS


def normals(x):
    """scipy.special.ndtri(clip(u, 1e-10, 1 - 1e-10)): gbm_qmc.py:36 as oracle/numpy_reference.py restates it."""
    from scipy.special import ndtri

    return ndtri(np.clip(uniforms(x), CLIP, 1 - CLIP))


def point_normals(sv, shift, first, count):
    """The normals matrix z (count, d) of points [first, first + count)."""
    return normals(points(sv, shift, np.arange(first, first + count, dtype=np.uint64)))


def index_where(sv_t, shift_t, target):
    """The k with x_t(k) = target, or None if the 30 direction numbers of the dimension are dependent: Gaussian elimination over
    GF(2) for the Gray code (which of the 30 numbers XOR to target ^ shift), then the Gray code inverted."""
    basis = {}                                     # leading bit -> (reduced direction number, the set of columns it is the XOR of)
    for b in range(BITS):
        v, cols = int(sv_t[b]), 1 << b
        while v and (v.bit_length() - 1) in basis:
            w, c = basis[v.bit_length() - 1]
            v, cols = v ^ w, cols ^ c
        if not v:
            return None
        basis[v.bit_length() - 1] = (v, cols)
    y, gray = int(target) ^ int(shift_t), 0
    while y:
        lead = y.bit_length() - 1
        if lead not in basis:
            return None
        w, c = basis[lead]
        y, gray = y ^ w, gray ^ c
    k = gray
    for s in (1, 2, 4, 8, 16):
        k ^= k >> s
    return k


def normal_chunks(d, n_points, seed, chunk, z=None):
    """Yields the normals of consecutive chunks of n_points points: of SciPy's Sobol(d, scramble=True, seed) from point 0 on (what
    the point-0 oracles always drew), or, where a matrix z (n_points, d) is given, its rows -- so one oracle serves any offset."""
    if z is not None:
        if z.shape != (n_points, d):
            raise ValueError(f"z is {z.shape}, expected {(n_points, d)}")
        for done in range(0, n_points, chunk):
            yield z[done:done + chunk]
        return
    from scipy.stats import norm, qmc

    eng = qmc.Sobol(d=d, scramble=True, seed=seed)
    done = 0
    while done < n_points:
        m = min(chunk, n_points - done)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            u = eng.random(m)
        yield norm.ppf(np.clip(u, CLIP, 1 - CLIP))
        done += m


def bridge_walk(z):
    """The pinned breadth-first Brownian bridge (include/olmc.h), over the rows of z (N, n): W (N, n + 1)."""
    n = z.shape[1]
    W = np.zeros((z.shape[0], n + 1))
    W[:, n] = math.sqrt(n) * z[:, 0]
    k = 1
    queue = collections.deque([(0, n)])
    while queue:
        a, b = queue.popleft()
        if b - a < 2:
            continue
        m = (a + b) // 2
        W[:, m] = ((b - m) * W[:, a] + (m - a) * W[:, b]) / (b - a) + math.sqrt((m - a) * (b - m) / (b - a)) * z[:, k]
        k += 1
        queue.append((a, m))
        queue.append((m, b))
    return W


def gbm_prices(z, bridge, S, T, r, sigma, q):
    """The price matrix (N, n + 1) of the normals z (N, n): ln S_j = ln S + j drift + vol W_j (exotic_options.py:54-67)."""
    m, n = z.shape
    dt = T / n
    drift, vol = (r - q - 0.5 * sigma**2) * dt, sigma * math.sqrt(dt)
    if bridge:
        W = bridge_walk(z)
    else:
        W = np.zeros((m, n + 1))
        W[:, 1:] = np.cumsum(z, axis=1)
    log_S = np.empty((m, n + 1))
    log_S[:, 0] = np.log(S)
    log_S[:, 1:] = np.log(S) + np.arange(1, n + 1) * drift + vol * W[:, 1:]
    return np.exp(log_S)
