"""The fp32 chains that sum a path's normals, replayed bit for bit from outside the device (not a test module).

Three kernels of olmc_kernels.h sum normals in fp32 before they widen to fp64:

  path_normal_quarters_walk / path_normal_sum   european_path_kernel in every mode and european_multi_kernel;
  cliquet_kernel                                the same block chain under a fold of its own (`part`, kSqrt2);
  asian_kernel<., true>                         the geometric average's prefix sums p and pp per 16 dates.

What pinned them was a relative 2e-6 on the price (tests/test_gpu_pair_sums.py, tests/test_gpu_parity.py, the REL class of
tests/test_gpu_exotics_reference_tie.py) -- a hundred times the chain's own rounding -- each other across launch shapes, and the parent's
bits.  Here the chain is stated exactly.  The hardware transcendentals cannot be reproduced on a CPU, but the instrumented build's
tap (tools.probe.binding.box_muller_probe) returns their results on chosen words, and everything after them is IEEE arithmetic:

  fp32 fma     tests/fp32_exact.fmaf    (one rounding; held against rational arithmetic by tests/test_fp32_exact_cpu.py)
  fp32 add     NumPy float32
  fp64 add     NumPy float64
  fp64 fma     tests/fp32_exact.fma     (Boldo and Melquiond's emulation, held against rational arithmetic in the same file; np.longdouble
                                         would not do: a 53 x 53-bit product needs 106 bits, x87 has 64)

The factors of a pair come from the existing tap alone (pair_factors): rad(xa) is the tap's z_cos at (xa, 0), s(xb) = sin(turns + 1/8)
its pair at (0x80000000, xb), where u_a = 1/2 and the radius is 1.  They are accepted only after two checks -- the tap returns exactly
1.0 at (0x80000000, 0) for z_cos and at (0x80000000, 0x00100000) for pair, and fl32(rad s) equals the tap's own pair(xa, xb) on EVERY
pair of the case, the sign of a zero aside -- and FactorsRefused is raised otherwise: a radius or a sine one ulp off fails the second
on about half of the pairs.

The replays are written from the kernels' comments and loop nests, not from the C checker, and are vectorised over paths (the control
flow of all three kernels is the same for every path).  tests/test_normal_sum_oracle_cpu.py holds each against a scalar transcription.
Words come from oracle.philox_oracle through tests/path_draw_oracle.philox_words; cases too large for its 25 us a block take
tests/box_muller_reference's vectorised generator, which the same CPU test holds equal to it.

The constants are the kernels' (olmc_kernels.h, olmc_host_math.h) and the host's products (olmc.hip: gbm_step, make_contract), by the
same Python float expressions.

Out of reach: asian_kernel<., false>, the arithmetic-fast Asian, takes v_exp_f32 on a rounded exponent and no tap returns it.  It stays
on its 2e-6.

Where the source adds a product to an fp64 accumulator (psum += kSqrt2 * part, a + vol * zsum) the replays take the form written: the
library is built with -ffp-contract=off (optionslab_amd/build.py), so a multiply and an add stay two roundings and only an explicit
__builtin_fma is one.  A build that contracted them would differ by 2^-53 of the product, which the GPU test's bound still covers.
"""
import math
from dataclasses import dataclass

import numpy as np

from tests import box_muller_reference as bm
from tests import fp32_exact as fx
from tests import path_draw_oracle as pdo

K_GROUP = 4                                        # kGroup: Philox blocks per fp32 chain
ASIAN_GROUP_DATES = 16                             # 4 * kAsianGroupBlocks
INV_SQRT2_F = np.float32(0.707106769)              # kInvSqrt2F
SQRT2 = 1.4142135623730951                         # kSqrt2
Z_SCALE = 1.1774100225154747                       # kZScale
PAIR_Z_SCALE = 1.6651092223153954                  # kPairZScale
assert Z_SCALE == math.sqrt(2.0 * math.log(2.0)) and INV_SQRT2_F == np.float32(1.0 / math.sqrt(2.0)) and SQRT2 == math.sqrt(2.0)
RAD_ONE = bm.RAD_ONE_WORD                          # u_a = 1/2: the radius is 1
QUARTER_AFTER_SHIFT = bm.EIGHTH_TURN               # x_b = 2^20: turns + 1/8 is a quarter turn, its sine 1
SMALL_CHAIN = 2.0 ** -18                           # a chain result below this resolves less than the GPU test asks for
F32, F64 = np.float32, np.float64


class FactorsRefused(AssertionError):
    """The tap's outputs are not the products of the factors read off it: `check` says which of the two checks failed."""

    def __init__(self, check, message):
        super().__init__(f"check {check}: {message}")
        self.check = check


@dataclass
class Factors:
    """Per Philox block the two pairs (x0, x1) and (x2, x3): every array [paths, blocks, 2], float32, RAW units."""
    rad: np.ndarray            # sqrt(-log2 u_a)
    s: np.ndarray              # sin(turns + 1/8 turn)
    pair: np.ndarray           # the tap's pair_sum_raw(0, xa, xb) = fl32(rad s)
    z_cos: np.ndarray          # the tap's box_muller_raw
    z_sin: np.ndarray

    @property
    def normals(self):
        """[paths, blocks, 4]: the RAW normals of steps 4b .. 4b + 3 (cos, sin, cos, sin)."""
        return np.stack([self.z_cos[..., 0], self.z_sin[..., 0], self.z_cos[..., 1], self.z_sin[..., 1]], axis=-1)


def tap_at_the_unit_points(tap):
    """(z_cos(0x80000000, 0), pair(0x80000000, 0x00100000)): what check 1 looks at."""
    z_cos, _z_sin, pair = tap(np.array([RAD_ONE, RAD_ONE], dtype=np.uint32), np.array([0, QUARTER_AFTER_SHIFT], dtype=np.uint32))
    return float(z_cos[0]), float(pair[1])


def pair_factors(tap, xa, xb):
    """(rad, s, pair, z_cos, z_sin), each float32 in the words' shape, after both checks; tap(xa, xb) -> (z_cos, z_sin, pair)."""
    xa, xb = np.asarray(xa, dtype=np.uint32), np.asarray(xb, dtype=np.uint32)
    shape = xa.shape
    xa, xb = xa.ravel(), xb.ravel()
    cos_one, pair_one = tap_at_the_unit_points(tap)
    if cos_one != 1.0 or pair_one != 1.0:
        raise FactorsRefused(1, f"z_cos(0x80000000, 0) = {cos_one!r}, pair(0x80000000, 0x00100000) = {pair_one!r}: not both 1.0")
    rad = np.asarray(tap(xa, np.zeros_like(xb))[0], dtype=F32)
    s = np.asarray(tap(np.full_like(xa, RAD_ONE), xb)[2], dtype=F32)
    z_cos, z_sin, pair = (np.asarray(o, dtype=F32) for o in tap(xa, xb))
    product = rad * s                                                              # float32 * float32: one rounding
    bad = ~(product == pair)                                                       # -0 == +0; a NaN equals nothing
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise FactorsRefused(2, f"fl32(rad s) is not the tap's pair on {int(bad.sum())} of {bad.size} pairs; first xa = {int(xa[i]):#010x}, "
                                f"xb = {int(xb[i]):#010x}: rad {rad[i]!r} s {s[i]!r} product {product[i]!r} pair {pair[i]!r}")
    return tuple(o.reshape(shape) for o in (rad, s, pair, z_cos, z_sin))


def block_factors(tap, words):
    """Factors of words[paths, blocks, 4]."""
    words = np.asarray(words, dtype=np.uint32)
    return Factors(*pair_factors(tap, words[..., 0::2], words[..., 1::2]))


def stand_in_tap(xa, xb):
    """A self-consistent tap without a device: fp32 rad, cos, sin and s from tests/box_muller_reference.py's fp64 values, and the
    outputs their fp32 products.  Not the device's transcendentals -- only arithmetic that factorises the way the kernels' does."""
    xb64 = np.asarray(xb, dtype=np.uint32).astype(np.int64)
    rad = bm.radius(xa).astype(F32)
    c, s = bm.cos_sin_turns(xb64)
    s8 = bm.cos_sin_turns(xb64 + bm.EIGHTH_TURN)[1]
    return rad * c.astype(F32), rad * s.astype(F32), rad * s8.astype(F32)


def case_words(seed, path_offset, count, blocks, tag=0):
    """words[count, blocks, 4] of paths [path_offset, path_offset + count)."""
    if count * blocks <= 1 << 16:
        return pdo.philox_words(seed, path_offset, count, blocks, tag)
    paths = np.uint64(path_offset) + np.arange(count, dtype=np.uint64)
    return np.stack([bm.philox_words(seed, paths, block=b, tag=tag) for b in range(blocks)], axis=1)


# ------------------------------------------------------------------------------------------------- the European sum ----
def _block_chain(acc, f, b):
    """raw_block_sum_of_words: fma(rad_b, s_b, fma(rad_a, s_a, acc)) on block b of every path."""
    acc = fx.fmaf(f.rad[:, b, 0], f.s[:, b, 0], acc)
    return fx.fmaf(f.rad[:, b, 1], f.s[:, b, 1], acc)


def quarter_groups(n_steps):
    """[(first group, end group)] of the quarters Q0 .. Q3: gq = ceil(n_groups / 4) groups each while they last."""
    n_groups = (n_steps >> 2) // K_GROUP
    gq = (n_groups + 3) >> 2
    return [(min(w * gq, n_groups), min((w + 1) * gq, n_groups)) for w in range(4)]


def european_zsum(words, n_steps, f, chains=None):
    """path_normal_sum of every path, float64 [paths]: the sum of the path's TRUE normals as the kernels form it.

    Full groups of K_GROUP blocks: an fp32 chain of eight fmas from 0.0f, cast to fp64 and added to its quarter (from 0.0, in order);
    ((Q0 + Q1) + Q2) + Q3 from 0.0; Q3 first takes the trailing full blocks as one fp32 chain and then the partial block -- n_steps % 4
    > 1: the first pair from 0.0f; n_steps % 4 odd: the z_cos of (x0, x1) (alone) or (x2, x3) (after the pair) through
    fmaf(z_cos, kInvSqrt2F, s) -- and the whole is multiplied by kPairZScale.  `chains`, a list, receives every fp32 chain result."""
    paths = words.shape[0]
    full = n_steps >> 2
    n_groups = full // K_GROUP
    assert words.shape[1] >= (n_steps + 3) >> 2 and f.rad.shape[:2] == words.shape[:2]
    keep = chains.append if chains is not None else (lambda s: None)
    acc = np.zeros(paths, dtype=F64)
    q = np.zeros(paths, dtype=F64)
    for w, (g0, g1) in enumerate(quarter_groups(n_steps)):
        q = np.zeros(paths, dtype=F64)
        for g in range(g0, g1):
            s = np.zeros(paths, dtype=F32)
            for j in range(K_GROUP):
                s = _block_chain(s, f, g * K_GROUP + j)
            keep(s)
            q = q + s.astype(F64)
        if w < 3:
            acc = acc + q
    b = n_groups * K_GROUP
    if b < full:
        s = np.zeros(paths, dtype=F32)
        for b in range(b, full):
            s = _block_chain(s, f, b)
        keep(s)
        q = q + s.astype(F64)
    rem = n_steps & 3
    if rem:
        s = np.zeros(paths, dtype=F32)
        if rem > 1:
            s = fx.fmaf(f.rad[:, full, 0], f.s[:, full, 0], s)
        if rem & 1:
            s = fx.fmaf(f.z_cos[:, full, 0 if rem == 1 else 1], INV_SQRT2_F, s)
        keep(s)
        q = q + s.astype(F64)
    acc = acc + q
    return acc * PAIR_Z_SCALE


# ------------------------------------------------------------------------------------------------------ the cliquet ----
def cliquet_period_sums(words, n_steps, n_periods, f, normals):
    """psum[paths, n_periods], float64: the RAW normal sum of every period as cliquet_kernel holds it when the period ends.

    Blocks with no reset date among their four steps (until_reset > 4) extend the fp32 chain `part` (pair-sum units); every K_GROUP such
    blocks, and before any block that holds a reset date, psum += kSqrt2 * part and the chain restarts from 0.0f.  In a block with a
    reset date the single RAW normals are added in fp64, the period closes where until_reset reaches 0 and psum restarts from 0.0.
    Steps beyond n_periods * (n_steps // n_periods) are never read."""
    paths = words.shape[0]
    steps_per_period = n_steps // n_periods
    used = steps_per_period * n_periods
    blocks = (used + 3) >> 2
    assert words.shape[1] >= blocks and normals.shape[:2] == words.shape[:2]
    out = []
    psum, part, part_blocks, until_reset = np.zeros(paths, dtype=F64), np.zeros(paths, dtype=F32), 0, steps_per_period
    for b in range(blocks):
        if until_reset > 4:
            until_reset -= 4
            part = _block_chain(part, f, b)
            part_blocks += 1
            if part_blocks == K_GROUP:
                psum = psum + SQRT2 * part.astype(F64)
                part, part_blocks = np.zeros(paths, dtype=F32), 0
            continue
        psum = psum + SQRT2 * part.astype(F64)
        part, part_blocks = np.zeros(paths, dtype=F32), 0
        for j in range(4):
            if 4 * b + j < used:
                psum = psum + normals[:, b, j].astype(F64)
                until_reset -= 1
                if until_reset == 0:
                    until_reset = steps_per_period
                    out.append(psum)
                    psum = np.zeros(paths, dtype=F64)
    assert len(out) == n_periods
    return np.stack(out, axis=1)


# --------------------------------------------------------------------------------------------- the geometric Asian ----
def geometric_asian_run(words, n_steps, normals, vol, drift):
    """(run_u, run_d), float64 [paths]: sum over the dates of ln(S_t / S_0) of the plain and of the mirrored leg, as asian_kernel<., true>
    leaves them.  vol = c.vol * kZScale (applied to RAW normals), drift per step.

    Per group of 16 dates (the last one open, with the dates that remain) fp32 prefix sums p += z, pp += p from 0.0f; close_group(n):
        run  += fma(+-vol, pp, fma(n, base, drift * n (n + 1) / 2)),      base += fma(+-vol, p, n * drift),
    in that order, all fp64, the casts of p and pp exact."""
    paths = words.shape[0]
    z = normals.reshape(paths, -1)
    assert z.dtype == F32 and z.shape[1] >= n_steps
    base = [np.zeros(paths, dtype=F64), np.zeros(paths, dtype=F64)]
    run = [np.zeros(paths, dtype=F64), np.zeros(paths, dtype=F64)]
    for start in range(0, n_steps, ASIAN_GROUP_DATES):
        n = min(ASIAN_GROUP_DATES, n_steps - start)
        p, pp = np.zeros(paths, dtype=F32), np.zeros(paths, dtype=F32)
        for t in range(start, start + n):
            p = p + z[:, t]
            pp = pp + p
        nd = float(n)
        tri = 0.5 * nd * (nd + 1.0)
        for leg, v in enumerate((vol, -vol)):
            run[leg] = run[leg] + fx.fma(v, pp.astype(F64), fx.fma(nd, base[leg], drift * tri))
            base[leg] = base[leg] + fx.fma(v, p.astype(F64), nd * drift)
    return run[0], run[1]


# ------------------------------------------------------------------------------------------------ what the host folds ----
def gbm_step(T, n_steps, r, q, sigma):
    """(dt, drift, vol) of olmc.hip's gbm_step."""
    dt = T / n_steps
    return dt, (r - q - 0.5 * sigma * sigma) * dt, sigma * math.sqrt(dt)


def contract(S, T, r, sigma, q, n_steps):
    """(a, vol) of make_contract: ln S_T = a +- vol zsum."""
    _dt, drift, vol = gbm_step(T, n_steps, r, q, sigma)
    return math.log(S) + drift * n_steps, vol


# ---------------------------------------------------------------------------------------------- bounds and resolution ----
def log_bound(log_s):
    """B = 8 x 2^-52 x max(1, |ln S_T|): what the device may add to the replayed logarithm of a terminal price.  One rounding each for
    vol zsum and for a + that (2^-53 |ln S_T| each, at most), the device exponential's documented 1 ulp (2^-52 relative on S_T, the
    same absolute on its logarithm) and the host logarithm that reads the price back (under 1 ulp of |ln S_T|, 2^-52): under
    3 x 2^-52 max(1, |ln S_T|), taken as 8 in the family of path_draw_oracle.gbm_bound's t + 8."""
    return 8.0 * 2.0 ** -52 * np.maximum(1.0, np.abs(np.asarray(log_s, dtype=F64)))


def resolution(chains, vol, log_s_both_legs):
    """(small, total, least): of the fp32 chain results of one case, how many are below SMALL_CHAIN in magnitude, how many there are,
    and over the others the least ratio of what one fp32 ulp of the chain moves ln S_T by -- vol kPairZScale ulp -- to the path's B
    (the larger of its two legs')."""
    b = np.max(log_bound(log_s_both_legs), axis=0)
    small, total, least = 0, 0, math.inf
    for s in chains:
        mag = np.abs(s.astype(F64))
        counted = mag >= SMALL_CHAIN
        small += int(np.sum(~counted))
        total += s.size
        if counted.any():
            ulp = np.spacing(np.abs(s[counted])).astype(F64)
            least = min(least, float(np.min(vol * PAIR_Z_SCALE * ulp / b[counted])))
    return small, total, least


# ------------------------------------------------------------------------------------- the cases of the GPU module ----
SEED = pdo.BIG_SEED                                # a non-zero high word
TERMINAL_STEPS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 63, 64, 65, 67, 80, 83, 252, 253, 255)
TERMINAL_PATHS = 321                               # five split workgroups, one live lane in the last
MIXED_SHAPE = (65_636, 17)                         # on 256 CUs: 256 whole workgroups and two split ones
SUM_PATHS, SUM_OFFSET = 257, (1 << 32) + 5
SUM_STEPS = (1, 2, 3, 16, 67, 83, 255)
MULTI_TAGS = (0, 1, 7, 0xFFFFFFFF)
CLIQUET_PERIODS = 3
CLIQUET_STEPS_PER_PERIOD = (1, 3, 4, 5, 16, 17, 21, 64, 67)
CLIQUET_TRAILING = (0, 2)
ASIAN_STEPS = (1, 3, 4, 15, 16, 17, 33, 64, 67, 252)

# The terminal prices: S = 1 and r - q = sigma^2 / 2 make a = 0, so ln S_T = +-vol zsum and B is 8 x 2^-52 for all but the tail paths;
# sigma sqrt(T) = 1 is as much volatility as leaves |ln S_T| near 1.  Both serve the resolution: a chain's ulp counts vol / max(1, |ln S_T|).
TERMINAL = dict(S=1.0, T=1.0, r=0.5, sigma=1.0, q=0.0)
# The sums: a call of strike 1 on a spot of 100 never clips (tests/test_gpu_box_muller.py).
SUMS = dict(S=100.0, K=1.0, T=1.0, r=0.05, sigma=0.2, q=0.01)
# The cliquet: no clip binds, and r = 0.6 with sigma = 0.05 puts every total 12 sigma above zero.
CLIQUET = dict(S=100.0, T=1.0, r=0.6, sigma=0.05, q=0.0, local_cap=1e9, local_floor=-2.0, global_cap=1e9, global_floor=-1e9)


def blocks_of(n_steps):
    return (n_steps + 3) >> 2
