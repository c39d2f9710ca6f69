"""Plain NumPy reference of the device's Box-Muller transform (not a test module).

The stream contract of include/olmc.h, evaluated in fp64 on the device's fp32 inputs:

    u_a    = fmaf((float) x_a, 2^-32, 2^-33)                 the one fp32 rounding the contract fixes (ua32)
    rad    = sqrt(-log2 u_a)                                 RAW units: a true normal is sqrt(2 ln 2) times this
    z_cos  = rad cos(2 pi t),  z_sin = rad sin(2 pi t),      t = (x_b & 0x7fffff) 2^-23 turns
    pair   = rad sin(2 pi t'),  t' = ((x_b + 2^20) & 0x7fffff) 2^-23      = (z_cos + z_sin) / sqrt(2)

and a vectorised Philox4x32-10 with the library's counter layout (path lo, path hi, block, tag; key = seed lo, seed hi), so that a
search over 2^26 paths for the words a seeded stream meets once in 2^25 draws takes seconds.  It also fixes the inputs, the strata and
the gate of tests/test_gpu_box_muller.py and tools/box_muller_accuracy.py, so that both measure the same thing.
"""
import math

import numpy as np

Z_SCALE = math.sqrt(2.0 * math.log(2.0))          # kZScale: RAW normal -> true normal
Z_SCALE_F32 = np.float32(1.17741002)               # kZScaleF of olmc_kernels.h
Z_ABS_TOL = 2e-5                                   # per-normal bound of tests/test_gpu_parity.py on typical draws
MANTISSA = 0x007FFFFF
EIGHTH_TURN = 1 << 20
ONE_WORDS = 0xFFFFFF80                             # x_a >= this: u_a rounds to exactly 1, the normal is an exact zero
TAIL_WORDS = 128                                   # x_a < this: u_a < 2^-25, |z| > 5.8

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
_LO, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


# ---------------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123's Philox4x32-10 on arrays of counters (any integer dtype, values < 2^32) and one key: four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c2 = (p1 >> _32) ^ c1 ^ np.uint64(k0), (p0 >> _32) ^ c3 ^ np.uint64(k1)
        c1, c3 = p1 & _LO, p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def philox_words(seed, paths, block=0, tag=0):
    """words[i, w] of global path paths[i] at one block of one stream: olmc_philox_words(seed, path, 1, block, 1, tag)[0, 0]."""
    paths = np.atleast_1d(np.asarray(paths, dtype=np.uint64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.stack(philox4x32_10(paths & _LO, paths >> _32, np.uint64(block), np.uint64(tag), seed & 0xFFFFFFFF, seed >> 32), axis=-1)


# ---------------------------------------------------------------------------------------------------- the transform
def ua32(xa):
    """The device's u_a as a float32 array: (float) x_a rounds to nearest, f 2^-32 + 2^-33 = (2 f + 1) 2^-33 is exact in fp64
    (2 f + 1 <= 2^33 + 1), and one rounding to fp32 makes it the fused multiply-add."""
    f = np.asarray(xa, dtype=np.uint32).astype(np.float32)
    return (f.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def radius(xa):
    return np.sqrt(-np.log2(ua32(xa).astype(np.float64)))


def cos_sin_turns(k):
    """(cos, sin)(2 pi k 2^-23) for integer lattice points k, exact zeros and ones on the quarter turns: the residual against the
    nearest quarter turn is exact in fp64, so the only errors are libm's on an argument within pi / 4."""
    t = (np.asarray(k, dtype=np.int64) & MANTISSA).astype(np.float64) * 2.0 ** -23
    quarter = np.rint(4.0 * t)
    a = 2.0 * np.pi * (t - 0.25 * quarter)
    c, s, q = np.cos(a), np.sin(a), quarter.astype(np.int64) & 3
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def raw(xa, xb):
    """(rad, z_cos, z_sin, pair) in fp64, RAW units."""
    xb = np.asarray(xb, dtype=np.uint32).astype(np.int64)
    rad = radius(xa)
    c, s = cos_sin_turns(xb)
    _, s8 = cos_sin_turns(xb + EIGHTH_TURN)
    return rad, rad * c, rad * s, rad * s8


def gate(rad):
    """The bound on Z_SCALE |device - reference| of one normal: a trigonometric error is absolute and is multiplied by the radius."""
    return Z_ABS_TOL * np.maximum(1.0, Z_SCALE * np.asarray(rad, dtype=np.float64))


def gate_ratio(dev, ref, rad):
    """Z_SCALE |dev - ref| / max(1, Z_SCALE rad): the gate is  ratio <= Z_ABS_TOL."""
    return Z_SCALE * np.abs(np.asarray(dev, dtype=np.float64) - ref) / np.maximum(1.0, Z_SCALE * rad)


# ---------------------------------------------------------------------------------------------------- the chosen inputs
RAD_ONE_WORD = 0x80000000                          # u_a = 1/2 exactly: rad = 1


def radius_edge_words():
    """0 .. 4095, 2^32 - 4096 .. 2^32 - 1 and 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 31."""
    powers = np.array([(1 << k) + d for k in range(1, 32) for d in (-1, 0, 1)], dtype=np.int64)
    return np.concatenate([np.arange(4096), np.arange((1 << 32) - 4096, 1 << 32), powers]).astype(np.uint32)


def radius_strided_words():
    """2^20 words 4096 j + 2049: every 2^-20 of the radius word's range."""
    return (4096 * np.arange(1 << 20, dtype=np.int64) + 2049).astype(np.uint32)


def angle_words():
    """(plain, random): the lattice angles -- 0, 1, the eight octants j 2^20 with their +-1 neighbours, 0x6FFFFF, 0x700000 and
    0x7FFFFF (where the eighth-turn add wraps) -- and 16 random words.  Every plain word w is also tested as w | 0xFF800000."""
    octants = [(j * EIGHTH_TURN + d) & MANTISSA for j in range(8) for d in (-1, 0, 1)]
    plain = np.array(sorted(set([0, 1, 0x6FFFFF, 0x700000, 0x7FFFFF] + octants)), dtype=np.uint32)
    return plain, np.random.default_rng(20240923).integers(0, 1 << 32, size=16, dtype=np.uint64).astype(np.uint32)


UPPER_NINE = np.uint32(0xFF800000)


ANGLE_STRATA = ("bulk", "lattice_zeros", "wrap_range")
RADIUS_STRATA = ("bulk", "tail_words", "near_one")


def angle_stratum(xb):
    """Index into ANGLE_STRATA: 'lattice_zeros' within one lattice point of an eighth turn (where v_sin / v_cos of the angle or of the
    shifted angle cross zero), 'wrap_range' for the other mantissas >= 0x700000 (the eighth-turn add carries out of the mantissa),
    else 'bulk'."""
    m = np.asarray(xb, dtype=np.int64) & MANTISSA
    near = ((m + 1) & (EIGHTH_TURN - 1)) <= 2
    return np.where(near, 1, np.where(m >= 0x700000, 2, 0)).astype(np.int8)


def radius_stratum(xa):
    """Index into RADIUS_STRATA: 'tail_words' x_a < 128, 'near_one' the top 4096 words (u_a within 2^-20 of 1), else 'bulk'."""
    x = np.asarray(xa, dtype=np.int64)
    return np.where(x < TAIL_WORDS, 1, np.where(x >= (1 << 32) - 4096, 2, 0)).astype(np.int8)


def _groups(codes, names):
    return {name: np.flatnonzero(codes == k) for k, name in enumerate(names) if (codes == k).any()}


def _fold_worst(into, groups, xa, xb, dev3, ref3, scale):
    """Fold one batch into `into`: {stratum: {output: dict(ratio, abs_err, xa, xb)}} keeps the worst gate ratio
    Z_SCALE |dev - ref| / max(1, Z_SCALE rad) of each output (scale = Z_SCALE / max(1, Z_SCALE rad)); not finite counts as inf."""
    for name, dev, ref in zip(("z_cos", "z_sin", "pair"), dev3, ref3):
        err = np.abs(dev - ref)                        # fp32 - fp64 -> fp64
        ratio = err * scale
        for stratum, idx in groups.items():
            i = idx[np.argmax(ratio[idx])]             # argmax returns a NaN's place if there is one
            r = float(ratio[i]) if np.isfinite(ratio[i]) else math.inf
            slot = into.setdefault(stratum, {}).setdefault(name, dict(ratio=-1.0))
            if r > slot["ratio"]:
                slot.update(ratio=r, abs_err=float(err[i]), xa=int(xa[i]), xb=int(xb[i]))
    return into


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def measure_angle_sweep(tap):
    """All 2^23 mantissas at rad = 1 through tap(xa, xb) -> (z_cos, z_sin, pair): dict(worst = per angle stratum, finite, upper_bits_ignored
    = the same outputs by bits with the upper nine bits of the angle word set, zeros_at_one = exact zeros at every angle for x_a = 2^32 - 1)."""
    k = np.arange(1 << 23, dtype=np.uint32)
    xa = np.full(k.size, RAD_ONE_WORD, dtype=np.uint32)
    dev = tap(xa, k)
    c, s = cos_sin_turns(k)
    s8 = np.roll(s, -EIGHTH_TURN)                      # sin at (k + 2^20) mod 2^23
    worst = _fold_worst({}, _groups(angle_stratum(k), ANGLE_STRATA), xa, k, dev, (c, s, s8), Z_SCALE / max(1.0, Z_SCALE))
    high = tap(xa, k | UPPER_NINE)
    at_one = tap(np.full(k.size, 0xFFFFFFFF, dtype=np.uint32), k)
    return dict(worst=worst, finite=all(bool(np.isfinite(d).all()) for d in dev),
                upper_bits_ignored=all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dev, high)),
                zeros_at_one=all(bool((d == 0.0).all()) for d in at_one))


def measure_radius_cross(tap, xa):
    """The radius words xa crossed with angle_words() through tap: dict(worst = per radius stratum, finite, upper_bits_ignored,
    zeros_at_one = all three outputs are zeros of either sign for x_a >= 0xFFFFFF80 at every angle, n = draws evaluated)."""
    xa = np.ascontiguousarray(xa, dtype=np.uint32)
    plain, rnd = angle_words()
    rad = radius(xa)
    scale = Z_SCALE / np.maximum(1.0, Z_SCALE * rad)
    groups, ones = _groups(radius_stratum(xa), RADIUS_STRATA), xa >= ONE_WORDS
    out = dict(worst={}, finite=True, upper_bits_ignored=True, zeros_at_one=True, n=0)
    for w in np.concatenate([plain, rnd]):
        xb = np.full(xa.size, w, dtype=np.uint32)
        dev = tap(xa, xb)
        (c,), (s,) = cos_sin_turns(np.array([w]))
        s8 = cos_sin_turns(np.array([int(w) + EIGHTH_TURN]))[1][0]
        _fold_worst(out["worst"], groups, xa, xb, dev, (rad * c, rad * s, rad * s8), scale)
        out["finite"] &= all(bool(np.isfinite(d).all()) for d in dev)
        out["zeros_at_one"] &= all(bool((d[ones] == 0.0).all()) for d in dev)
        out["n"] += xa.size
        if w in plain:
            high = tap(xa, xb | UPPER_NINE)
            out["upper_bits_ignored"] &= all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dev, high))
    return out


# ---------------------------------------------------------------------------------------------------- one path of the product
def path_normals(seed, path, n_steps):
    """(z, rad): the n_steps TRUE reference normals (fp64) of one global path and the RAW radius each was drawn with -- words
    (x0, x1) of block b make steps 4b (cos) and 4b + 1 (sin), (x2, x3) steps 4b + 2 and 4b + 3."""
    z, rads = [], []
    for b in range((n_steps + 3) // 4):
        w = philox_words(seed, [path], block=b)[0]
        for xa, xb in ((w[0], w[1]), (w[2], w[3])):
            rad, c, s, _ = raw(np.array([xa], dtype=np.uint32), np.array([xb], dtype=np.uint32))
            z += [Z_SCALE * c[0], Z_SCALE * s[0]]
            rads += [rad[0], rad[0]]
    return np.array(z[:n_steps]), np.array(rads[:n_steps])


def gbm_spots(z, S, T, r, sigma, q=0.0):
    """S_1 .. S_n of the exact GBM step on the normals z (src/simulation/gbm_numpy.py:35-51)."""
    dt = T / len(z)
    return S * np.exp(np.cumsum((r - q - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * np.asarray(z, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------------- sqrt_nonneg
def sqrt_inputs():
    """{range: x} for the Heston kernels' square root: the claimed range [1e-12, 10] (400,000 log-uniform points), exact squares
    k^2 2^-40, the ranges beside it down to 1e-30 and up to 1e30, and what lies below 1e-30 (subnormals included)."""
    rng = np.random.default_rng(11)
    k = np.arange(1, 4097, dtype=np.float64)
    return dict(claimed=10.0 ** rng.uniform(-12.0, 1.0, 400_000), squares=k * k * 2.0 ** -40,
                below=np.concatenate([10.0 ** rng.uniform(-30.0, -12.0, 100_000), [1e-30, np.nextafter(1e-12, 0.0)]]),
                above=np.concatenate([10.0 ** rng.uniform(1.0, 30.0, 100_000), [np.nextafter(10.0, 11.0), 1e30]]),
                tiny=np.concatenate([10.0 ** rng.uniform(-307.0, -30.0, 50_000), [5e-324, 2.2250738585072014e-308, 1e-45, 1.1754943508222875e-38,
                                                                                   np.nextafter(1e-30, 0.0)]]))


def measure_sqrt(tap):
    """{range: dict(ulp, rel, abs_err, x = where the ulp error is worst, finite, non_negative)} of tap(x) against numpy.sqrt."""
    out = {}
    for name, x in sqrt_inputs().items():
        y, want = tap(x), np.sqrt(x)
        err = np.abs(y - want)
        ulp = err / np.spacing(want)
        i = int(np.argmax(ulp))
        out[name] = dict(ulp=float(ulp[i]), rel=float((err / want).max()), abs_err=float(err.max()), x=float(x[i]),
                         finite=bool(np.isfinite(y).all()), non_negative=bool((y >= 0.0).all()))
    return out
