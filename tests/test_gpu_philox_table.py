"""The Philox prefix table of the European launches (olmc_kernels.h: PhiloxPrefix, OLMC_TUNE_PHILOX_TABLE).

A launch whose grid covers every path, whose paths have at most 64 Philox blocks and share the high word of the path index takes
the three words per block that all its paths share after Philox rounds 1-2 from a table the host builds per launch; every other
launch runs all ten rounds per thread.  The words are the same words, and the association of every sum is untouched, so the table
must not show in a single bit: terminal arrays byte-identical, every sum equal, with the knob on and off -- at every remainder of
n_steps modulo 4 and 16, the last table entry, the shapes with whole, split and partly dead workgroups, both antithetic settings,
a high path word of 1, and seeds with a non-zero high word.  Which launches carry a table is asserted on the instrumented build
(OLMC_PROBE_TUNE_EXPECT_TABLE): 257 and 1024 steps, a grid-striding launch and a launch that straddles a multiple of 2^32 run the
same code under both settings."""
import pytest

from optionslab_amd import _hip
from tools.probe import binding as probe

pytestmark = pytest.mark.gpu

S, K, T, R, V, Q = 100.0, 105.0, 1.0, 0.05, 0.2, 0.01
TABLE_STEPS = [4, 5, 7, 16, 63, 64, 67, 252, 255, 256]       # every remainder mod 4, partial groups, 64 blocks with and without a partial one
FALLBACK_STEPS = [257, 1024]                                 # 65 and 256 blocks: no table
PATHS = [1, 63, 64, 255, 256, 257, 1000, 70_000]             # 70,000 = whole + split workgroups on 256 compute units
SEEDS = [0x9E3779B97F4A7C15, (7 << 32) | 42]                 # both with a non-zero high word
TWO32 = 1 << 32


def first_order(S_=S):
    return [(S_, K, T, R, V, Q, True), (S_ + 1, K, T, R, V, Q, True), (S_ - 1, K, T, R, V, Q, True), (S_, K, T, R, V + 0.01, Q, True),
            (S_, K, T, R, V - 0.01, Q, True), (S_, K, T - 1 / 365.0, R, V, Q, True), (S_, K, T, R + 1e-4, V, Q, True), (S_, K, T, R - 1e-4, V, Q, True)]


FOURTEEN = first_order() + [(S + 1, K, T, R, V + 0.01, Q, False), (S - 1, K, T, R, V - 0.01, Q, False), (S, K, T, R, V + 0.02, Q, True),
                            (S, K, T, R, V - 0.02, Q, True), (S + 2, K, T, R, V, Q, False), (S - 2, K, T, R, V, Q, False)]


class knob:
    """`with knob(hip, table, split)`: OLMC_TUNE_PHILOX_TABLE and OLMC_TUNE_SPLIT_TAIL of one library, restored on exit."""

    def __init__(self, hip, table, split=0):
        self.hip, self.table, self.split = hip, table, split

    def __enter__(self):
        self.hip.tune(self.hip.TUNE_PHILOX_TABLE, self.table)
        self.hip.tune(self.hip.TUNE_SPLIT_TAIL, self.split)

    def __exit__(self, *exc):
        self.hip.tune(self.hip.TUNE_PHILOX_TABLE, 1)
        self.hip.tune(self.hip.TUNE_SPLIT_TAIL, 0)


def sums(hip, n, m, seed, anti, offset=0):
    """Every reduced quantity the table reaches: one contract, the 8- and 16-wide fused kernels with both sums and sum-only, the
    control variate."""
    st = hip.european(S, K, T, R, V, Q, True, n, m, seed, anti, path_offset=offset)
    out = [st.sum, st.sumsq, st.n]
    for opts in (first_order(), FOURTEEN):
        out += [x for e in hip.european_batch(opts, n, m, seed, anti, path_offset=offset) for x in (e.sum, e.sumsq)]
    cv = hip.european_cv_shard(S, K, T, R, V, Q, True, offset, n, m, seed, anti)
    out += [cv.sum_d, cv.sum_s, cv.sum_dd, cv.sum_ss, cv.sum_ds]
    if offset == 0 and anti:                                  # the Greeks entry point is antithetic and starts at path 0
        for second in (False, True):
            out += hip.european_greeks_fd(S, K, T, R, V, Q, True, n, m, seed, second, want_evals=False)[0]      # sum-only kernels
    return out


@pytest.mark.parametrize("split", [0, -1], ids=["split", "whole"])
@pytest.mark.parametrize("anti", [True, False], ids=["antithetic", "plain"])
def test_terminal_prices_are_the_same_bytes_with_and_without_the_table(anti, split):
    """olmc_european_terminal at every (n_steps, n_paths, seed): below 64 steps nothing splits, from 64 on the small launches are all
    split workgroups by default and all whole ones with OLMC_TUNE_SPLIT_TAIL = -1; 70,000 paths have both kinds in one launch."""
    for m in TABLE_STEPS + FALLBACK_STEPS:
        for n in PATHS:
            for seed in SEEDS:
                with knob(_hip, 1, split):
                    on = _hip.european_terminal(S, T, R, V, Q, n, m, seed, anti)
                with knob(_hip, 0, split):
                    off = _hip.european_terminal(S, T, R, V, Q, n, m, seed, anti)
                assert on.tobytes() == off.tobytes(), (m, n, hex(seed))


@pytest.mark.parametrize("split", [0, -1], ids=["split", "whole"])
@pytest.mark.parametrize("anti", [True, False], ids=["antithetic", "plain"])
def test_every_sum_is_the_same_with_and_without_the_table(anti, split):
    for m in TABLE_STEPS + FALLBACK_STEPS:
        for n in (1, 257, 1000, 70_000):
            seed = SEEDS[(m + n) & 1]
            with knob(_hip, 1, split):
                on = sums(_hip, n, m, seed, anti)
            with knob(_hip, 0, split):
                off = sums(_hip, n, m, seed, anti)
            assert on == off, (m, n, hex(seed))              # equal bits (no NaN among them: NaN would compare unequal)


def expect(value):
    """Sets OLMC_PROBE_TUNE_EXPECT_TABLE on the instrumented build; raises if a launch since the last setting did otherwise."""
    probe.tune(probe.TUNE_EXPECT_TABLE, value)


def test_which_launches_carry_a_table():
    """On the instrumented build (the product's own translation unit): with the knob on, launches of up to 256 steps carry a table and
    those of 257 and 1024 steps, a grid-striding launch (more than 4096 workgroups of at most 128 steps) and a launch across a
    multiple of 2^32 paths do not; with the knob off none does -- so the fallback shapes run the same code under both settings."""
    hip = probe.hip
    seed = SEEDS[0]
    expect(0)
    try:
        for table in (1, 0):
            with knob(hip, table):
                expect(1 if table else -1)
                for m in TABLE_STEPS:
                    for n in (1, 257, 70_000):
                        sums(hip, n, m, seed, True)
                        hip.european_terminal(S, T, R, V, Q, n, m, seed, False)
                sums(hip, 300, 252, seed, True, offset=TWO32 + 5)
                expect(-1)                                   # raises if one of the launches above did not meet the expectation
                for m in FALLBACK_STEPS:
                    sums(hip, 257, m, seed, True)
                    hip.european_terminal(S, T, R, V, Q, 1000, m, seed, True)
                sums(hip, 1_100_000, 4, seed, True)          # 4,297 workgroups' worth of paths on 4,096 grid-striding workgroups
                sums(hip, 300, 252, seed, True, offset=TWO32 - 100)
                expect(0)
    finally:
        hip.tune(hip.TUNE_PHILOX_TABLE, 1)
        try:
            expect(0)
        except Exception:
            pass


def test_a_grid_striding_launch_is_untouched():
    on = sums(_hip, 1_100_000, 4, SEEDS[1], True)
    with knob(_hip, 0):
        off = sums(_hip, 1_100_000, 4, SEEDS[1], True)
    assert on == off


@pytest.mark.parametrize("anti", [True, False], ids=["antithetic", "plain"])
@pytest.mark.parametrize("m", [7, 252])
def test_the_high_path_word(m, anti):
    """path_offset = 2^32 + 5: every path has high word 1, which the table must carry (the knob-off launch forms it per lane).
    path_offset = 2^32 - 100 with 300 paths straddles the boundary: no table, the same sums under both settings, and the sums of a
    launch split at the boundary.  The two parts group the same per-path values into other workgroup rows, so they agree to the
    reassociation of an fp64 sum of n <= 600 non-negative terms, (n - 1) * 2^-53 relative = 6.7e-14: the bound is 1e-13."""
    seed = SEEDS[1]
    above = sums(_hip, 300, m, seed, anti, offset=TWO32 + 5)
    straddle = sums(_hip, 300, m, seed, anti, offset=TWO32 - 100)
    low, high = sums(_hip, 100, m, seed, anti, offset=TWO32 - 100), sums(_hip, 200, m, seed, anti, offset=TWO32)
    with knob(_hip, 0):
        assert sums(_hip, 300, m, seed, anti, offset=TWO32 + 5) == above
        assert sums(_hip, 300, m, seed, anti, offset=TWO32 - 100) == straddle
        assert sums(_hip, 200, m, seed, anti, offset=TWO32) == high
    assert above != straddle
    for whole, a, b in zip(straddle, low, high):
        assert whole == pytest.approx(a + b, rel=1e-13, abs=0.0)
