"""tests/normal_sum_oracle.py without a device: through a self-consistent stand-in tap (fp32 rad, s, cos from
tests/box_muller_reference.py; z_cos = fl32(rad cos), pair = fl32(rad s)) the factor extraction, each vectorised replay against a
scalar transcription of the kernel's loop nest, the coverage of the quarters, and the resolution of the GPU module's bound.

The scalar transcriptions below follow olmc_kernels.h line by line (path_normal_quarters_walk, cliquet_kernel, asian_kernel<., true>) in
Python floats (fp64) and numpy.float32 scalars, with an fmaf and an fma of their own: rational arithmetic, rounded once.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import box_muller_reference as bm
from tests import normal_sum_oracle as nso
from tests import path_draw_oracle as pdo
from tests.test_fp32_exact_cpu import round_fraction

F32 = np.float32
PATHS = 64


@pytest.fixture(scope="module")
def stand_in():
    """(words, factors) of 64 paths over every block any case reads."""
    blocks = nso.blocks_of(max(max(nso.TERMINAL_STEPS), max(nso.ASIAN_STEPS), nso.CLIQUET_PERIODS * max(nso.CLIQUET_STEPS_PER_PERIOD) + 2))
    words = nso.case_words(nso.SEED, nso.SUM_OFFSET, PATHS, blocks)
    return words, nso.block_factors(nso.stand_in_tap, words)


# ----------------------------------------------------------------------------------------------------- the factors ----
def test_factor_extraction_returns_the_stand_ins_radius_and_sine_bit_for_bit(stand_in):
    words, f = stand_in
    xa, xb = words[..., 0::2], words[..., 1::2]
    want_rad = bm.radius(xa).astype(F32)
    want_s = bm.cos_sin_turns(xb.astype(np.int64) + bm.EIGHTH_TURN)[1].astype(F32)
    assert np.array_equal(f.rad.view(np.uint32), want_rad.view(np.uint32))
    assert np.array_equal(f.s.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(f.pair, want_rad * want_s)
    assert nso.tap_at_the_unit_points(nso.stand_in_tap) == (1.0, 1.0)
    assert f.normals.shape == words.shape and np.array_equal(f.normals[..., 2], f.z_cos[..., 1])


def test_a_radius_read_one_ulp_off_fails_the_second_check(stand_in):
    words, _f = stand_in

    def off_by_an_ulp(xa, xb):
        z_cos, z_sin, pair = nso.stand_in_tap(xa, xb)
        reads_a_radius = ((np.asarray(xb) & bm.MANTISSA) == 0) & (np.asarray(xa) != nso.RAD_ONE)
        return np.where(reads_a_radius, np.nextafter(z_cos, F32(np.inf)), z_cos), z_sin, pair

    assert nso.tap_at_the_unit_points(off_by_an_ulp) == (1.0, 1.0)                 # the first check cannot see it
    with pytest.raises(nso.FactorsRefused) as refused:
        nso.block_factors(off_by_an_ulp, words)
    assert refused.value.check == 2


def test_a_tap_that_is_not_one_at_the_unit_points_fails_the_first_check(stand_in):
    words, _f = stand_in

    def short_of_one(xa, xb):
        z_cos, z_sin, pair = nso.stand_in_tap(xa, xb)
        return z_cos, z_sin, np.where(pair == 1.0, np.nextafter(F32(1.0), F32(0.0)), pair)

    with pytest.raises(nso.FactorsRefused) as refused:
        nso.block_factors(short_of_one, words)
    assert refused.value.check == 1


def test_the_vectorised_words_are_the_integer_oracles():
    """case_words takes tests/box_muller_reference's generator for the large case: the same words, also beyond 2^32 and on a tag."""
    for offset, tag in ((0, 0), (nso.SUM_OFFSET, 7), (65_530, 0xFFFFFFFF)):
        paths = np.uint64(offset) + np.arange(40, dtype=np.uint64)
        got = np.stack([bm.philox_words(nso.SEED, paths, block=b, tag=tag) for b in range(5)], axis=1)
        assert np.array_equal(got, pdo.philox_words(nso.SEED, offset, 40, 5, tag))
    big = nso.case_words(nso.SEED, 0, *[nso.MIXED_SHAPE[0], nso.blocks_of(nso.MIXED_SHAPE[1])])
    assert big.shape == (nso.MIXED_SHAPE[0], 5, 4) and np.array_equal(big[-40:], pdo.philox_words(nso.SEED, nso.MIXED_SHAPE[0] - 40, 40, 5, 0))


# ------------------------------------------------------------------------------------------ scalar transcriptions ----
def _exact(x):
    return Fraction(float(x))


def fmaf(a, b, c):
    return F32(float(round_fraction(_exact(a) * _exact(b) + _exact(c), 24)))


def fma(a, b, c):
    return float(round_fraction(_exact(a) * _exact(b) + _exact(c), 53))


def scalar_european(f, i, n_steps):
    def pair_sum_raw(acc, b, k):
        return fmaf(f.rad[i, b, k], f.s[i, b, k], acc)

    def raw_block_sum(acc, b):
        return pair_sum_raw(pair_sum_raw(acc, b, 0), b, 1)

    full = n_steps >> 2
    n_groups = full // 4
    gq = (n_groups + 3) >> 2
    acc, q = 0.0, 0.0
    for w in range(0, 4):
        q = 0.0
        b1 = min((w + 1) * gq, n_groups) * 4
        b = min(w * gq, n_groups) * 4
        while b < b1:
            s = F32(0.0)
            for j in range(4):
                s = raw_block_sum(s, b + j)
            q += float(s)
            b += 4
        if w < 3:
            acc += q
    b = n_groups * 4
    if b < full:
        s = F32(0.0)
        while b < full:
            s = raw_block_sum(s, b)
            b += 1
        q += float(s)
    rem = n_steps & 3
    if rem:
        s = F32(0.0)
        if rem > 1:
            s = pair_sum_raw(F32(0.0), full, 0)
        if rem & 1:
            s = fmaf(f.z_cos[i, full, 0 if rem == 1 else 1], nso.INV_SQRT2_F, s)
        q += float(s)
    acc += q
    return acc * nso.PAIR_Z_SCALE


def scalar_cliquet(f, z, i, n_steps, n_periods):
    steps_per_period = n_steps // n_periods
    used_steps = steps_per_period * n_periods
    out = []
    psum, part, part_blocks, until_reset = 0.0, F32(0.0), 0, steps_per_period
    for b in range((used_steps + 3) >> 2):
        if until_reset > 4:
            until_reset -= 4
            part = fmaf(f.rad[i, b, 1], f.s[i, b, 1], fmaf(f.rad[i, b, 0], f.s[i, b, 0], part))
            part_blocks += 1
            if part_blocks == 4:
                psum += nso.SQRT2 * float(part)
                part, part_blocks = F32(0.0), 0
            continue
        psum += nso.SQRT2 * float(part)
        part, part_blocks = F32(0.0), 0
        for j in range(4):
            if 4 * b + j < used_steps:
                psum += float(z[i, b, j])
                until_reset -= 1
                if until_reset == 0:
                    until_reset = steps_per_period
                    out.append(psum)
                    psum = 0.0
    return out


def scalar_asian(z, i, n_steps, vol, drift):
    full, rem = n_steps >> 2, n_steps & 3
    base_u = base_d = run_u = run_d = 0.0
    p, pp = F32(0.0), F32(0.0)

    def block(b, live):
        nonlocal p, pp
        for j in range(live):
            p = p + z[i, b, j]
            pp = pp + p

    def close_group(n):
        nonlocal base_u, base_d, run_u, run_d, p, pp
        nd = float(n)
        tri = 0.5 * nd * (nd + 1.0)
        run_u += fma(vol, float(pp), fma(nd, base_u, drift * tri))
        run_d += fma(-vol, float(pp), fma(nd, base_d, drift * tri))
        base_u += fma(vol, float(p), nd * drift)
        base_d += fma(-vol, float(p), nd * drift)
        p, pp = F32(0.0), F32(0.0)

    b = 0
    while b + 4 <= full:
        for k in range(4):
            block(b + k, 4)
        close_group(16)
        b += 4
    tail_blocks = full - b
    for k in range(4):
        if k < tail_blocks:
            block(b + k, 4)
        elif k == tail_blocks and rem:
            block(full, rem)
    open_dates = 4 * tail_blocks + rem
    if open_dates:
        close_group(open_dates)
    return run_u, run_d


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("n_steps", nso.TERMINAL_STEPS)
def test_the_european_replay_is_the_kernels_loop_nest(stand_in, n_steps):
    words, f = stand_in
    chains = []
    got = nso.european_zsum(words, n_steps, f, chains)
    assert got.dtype == np.float64 and _same_bits(got, [scalar_european(f, i, n_steps) for i in range(PATHS)])
    full = n_steps >> 2
    assert len(chains) == full // 4 + (full % 4 != 0) + (n_steps % 4 != 0) and all(c.dtype == F32 for c in chains)
    # in units of its own rounding the replay is the fp64 sum of the stand-in's normals (what tests/test_gpu_pair_sums.py compares with)
    z = f.normals.reshape(PATHS, -1)[:, :n_steps].astype(np.float64).sum(axis=1) * nso.Z_SCALE
    assert np.max(np.abs(got - z)) <= 4e-6 * math.sqrt(n_steps)


@pytest.mark.parametrize("trailing", nso.CLIQUET_TRAILING)
@pytest.mark.parametrize("steps_per_period", nso.CLIQUET_STEPS_PER_PERIOD)
def test_the_cliquet_replay_is_the_kernels_loop_nest(stand_in, steps_per_period, trailing):
    words, f = stand_in
    n_steps = nso.CLIQUET_PERIODS * steps_per_period + trailing
    assert n_steps // nso.CLIQUET_PERIODS == steps_per_period
    got = nso.cliquet_period_sums(words, n_steps, nso.CLIQUET_PERIODS, f, f.normals)
    assert got.shape == (PATHS, nso.CLIQUET_PERIODS)
    assert _same_bits(got, [scalar_cliquet(f, f.normals, i, n_steps, nso.CLIQUET_PERIODS) for i in range(PATHS)])
    z = f.normals.reshape(PATHS, -1)[:, :nso.CLIQUET_PERIODS * steps_per_period].astype(np.float64)
    assert np.max(np.abs(got - z.reshape(PATHS, nso.CLIQUET_PERIODS, steps_per_period).sum(axis=2))) <= 4e-6 * math.sqrt(steps_per_period)
    if trailing:                                                                    # trailing steps are never read
        poisoned = nso.Factors(*(np.where(np.arange(words.shape[1])[None, :, None] * 4 >= n_steps - trailing, F32(np.nan), a)
                                 for a in (f.rad, f.s, f.pair, f.z_cos, f.z_sin)))
        assert np.isfinite(nso.cliquet_period_sums(words, n_steps, nso.CLIQUET_PERIODS, poisoned, poisoned.normals)).all()


@pytest.mark.parametrize("n_steps", nso.ASIAN_STEPS)
def test_the_geometric_asian_replay_is_the_kernels_loop_nest(stand_in, n_steps):
    words, f = stand_in
    _dt, drift, vol = nso.gbm_step(nso.SUMS["T"], n_steps, nso.SUMS["r"], nso.SUMS["q"], nso.SUMS["sigma"])
    vol = vol * nso.Z_SCALE
    run_u, run_d = nso.geometric_asian_run(words, n_steps, f.normals, vol, drift)
    want = [scalar_asian(f.normals, i, n_steps, vol, drift) for i in range(PATHS)]
    assert _same_bits(run_u, [w[0] for w in want]) and _same_bits(run_d, [w[1] for w in want])
    cum = np.cumsum(vol * f.normals.reshape(PATHS, -1)[:, :n_steps].astype(np.float64) + drift, axis=1).sum(axis=1)
    assert np.max(np.abs(run_u - cum)) <= 1e-5 * n_steps


# ------------------------------------------------------------------------------------------------------- coverage ----
@pytest.mark.parametrize("n_steps", sorted(set(nso.TERMINAL_STEPS + nso.SUM_STEPS + (nso.MIXED_SHAPE[1],))))
def test_the_quarters_and_the_tail_cover_every_full_block_once(n_steps):
    full = n_steps >> 2
    n_groups = full // nso.K_GROUP
    quarters = nso.quarter_groups(n_steps)
    blocks = [g * nso.K_GROUP + j for g0, g1 in quarters for g in range(g0, g1) for j in range(nso.K_GROUP)]
    blocks += list(range(n_groups * nso.K_GROUP, full))
    assert blocks == list(range(full))
    assert len(quarters) == 4 and all(g1 - g0 <= (n_groups + 3) // 4 for g0, g1 in quarters)
    if n_groups == 5:
        assert [g1 - g0 for g0, g1 in quarters] == [2, 2, 1, 0]
    if n_groups == 15:
        assert [g1 - g0 for g0, g1 in quarters] == [4, 4, 4, 3]


def test_the_step_counts_take_every_branch_of_the_walk():
    groups = {(n >> 2) // nso.K_GROUP for n in nso.TERMINAL_STEPS}
    assert {0, 1, 4, 5, 15} <= groups                                               # none, one, one per quarter, uneven quarters
    assert {n & 3 for n in nso.TERMINAL_STEPS} == {0, 1, 2, 3}
    assert any((n >> 2) % nso.K_GROUP and (n >> 2) >= nso.K_GROUP for n in nso.TERMINAL_STEPS)   # trailing blocks after full groups
    assert any((n >> 2) == 0 for n in nso.TERMINAL_STEPS)


# ----------------------------------------------------------------------------------------------------- resolution ----
def test_one_ulp_of_a_chain_is_a_hundred_times_the_gpu_bound_on_the_stand_in():
    """Moving one fp32 chain result of one path by one ulp moves ln S_T by vol kPairZScale ulp: at least 100 B for every chain of the
    terminal-price cases that is not below 2^-18 in magnitude, and at most 1 chain in 10,000 of any case is (the chains' density at
    zero, 0.166, gives 1.3e-6).  The figure is that of the case's own chains: a chain just above 2^-18 would resolve only about
    vol kPairZScale 2^-41 / B, which no volatility makes a hundred at 255 steps; the smallest chain the cases hold is far larger."""
    words = nso.case_words(nso.SEED, 0, nso.TERMINAL_PATHS, nso.blocks_of(max(nso.TERMINAL_STEPS)))
    f = nso.block_factors(nso.stand_in_tap, words)
    for n_steps in nso.TERMINAL_STEPS:
        chains = []
        zsum = nso.european_zsum(words, n_steps, f, chains)
        a, vol = nso.contract(n_steps=n_steps, **nso.TERMINAL)
        assert a == 0.0
        small, total, least = nso.resolution(chains, vol, np.stack([a + vol * zsum, a - vol * zsum]))
        assert small * 10_000 <= total, (n_steps, small, total)
        assert least >= 100.0, (n_steps, least)
