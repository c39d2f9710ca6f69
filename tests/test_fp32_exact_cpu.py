"""tests/fp32_exact.py against rational arithmetic (fractions): one rounding, also where two roundings differ.

fp32 subnormal results are out of scope (fp32_exact's docstring): every triple here has a result of at least 2^-100 in magnitude or an
exact zero.  The fp64 sibling is held the same way on operands of the kernels' size.
"""
from fractions import Fraction

import numpy as np

from tests import fp32_exact as fx


def round_fraction(r, bits):
    """The Fraction r rounded to `bits` significant bits, ties to even, as a Fraction (no exponent limits)."""
    if r == 0:
        return Fraction(0)
    e = abs(r).numerator.bit_length() - abs(r).denominator.bit_length()            # 2^(e - 1) < |r| < 2^(e + 1)
    if abs(r) < Fraction(2) ** e:
        e -= 1                                                                      # 2^e <= |r| < 2^(e + 1)
    ulp = Fraction(2) ** (e - bits + 1)
    return round(r / ulp) * ulp                                                     # Fraction.__round__: half to even


def exact_fmaf(a, b, c):
    return [round_fraction(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)), 24) for x, y, z in zip(a, b, c)]


def naive_fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chain_triples(rng, n):
    """The operands of pair_sum_raw: a radius up to 5.75, a sine, an accumulator below 100."""
    return (rng.uniform(0.0, 5.75, n).astype(np.float32), rng.uniform(-1.0, 1.0, n).astype(np.float32),
            (rng.uniform(-100.0, 100.0, n) * 10.0 ** rng.uniform(-6.0, 0.0, n)).astype(np.float32))


def cancelling_triples(rng, n):
    """c = -fl32(a b): the result is the product's own rounding error, exact."""
    a, b = rng.uniform(-5.75, 5.75, n).astype(np.float32), rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return a, b, -(a * b)


def scaled_triples(rng, n):
    """Operands whose exponents lie far apart (a result stays above 2^-100)."""
    def draw():
        return (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-25, 26, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return draw(), draw(), draw()


def tie_triples(rng, n):
    """(a, b, c, side): a b + c = h + side u, h = (2 m + 1) 2^-24 an fp32 halfway point in [1, 2) and u the last place of the exact sum.

    (k 2^x - 1)(k 2^x + 1) = k^2 2^(2x) - 1 with k odd and 2x >= 30 is a 48-bit product one unit short of k^2 2^(2x): scaled by
    2^(-24 - 2x) it is Q - u with Q = k^2 2^-24 and u = 2^(-24 - 2x) <= 2^-54, far below the fp64 ulp 2^-52 of the sum.  So
        side  0:  a = b' = k 2^x (the product is Q),      c = h - Q
        side -1:  a b = Q - u,                             c = h - Q
        side +1:  a b = -(Q - u),                          c = h + Q
    and c = (2 m + 1 -+ k^2) 2^-24 is an even multiple of 2^-24 below 2^25 of them: an fp32 value.  float64(a) * b + c rounds to h in all
    three, and the cast to fp32 then takes the even neighbour whatever the side."""
    x = rng.integers(15, 24, n)
    k = 2 * rng.integers(0, 2 ** (24 - x) // 2, n) + 1                              # odd, k 2^x + 1 < 2^24, k^2 < 2^18
    m = rng.integers(2 ** 23, 2 ** 24 - 2 ** 18, n)
    side = rng.integers(-1, 2, n)
    scale = 2.0 ** (-24.0 - 2.0 * x)
    big = (k * 2 ** x).astype(np.float64)
    a = np.where(side == 0, big, big - 1.0) * scale
    b = np.where(side == 0, big, big + 1.0) * np.where(side == 1, -1.0, 1.0)
    c = (2.0 * m + 1.0 + np.where(side == 1, 1.0, -1.0) * (k * k).astype(np.float64)) * 2.0 ** -24
    a32, b32, c32 = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    assert np.array_equal(a32, a) and np.array_equal(b32, b) and np.array_equal(c32, c)
    return a32, b32, c32, side, m


def _assert_exact(a, b, c, label):
    got = fx.fmaf(a, b, c)
    assert got.dtype == np.float32 and got.shape == a.shape
    want = exact_fmaf(a, b, c)
    bad = [i for i in range(a.size) if Fraction(float(got[i])) != want[i]]
    assert not bad, (label, len(bad), [(a[i], b[i], c[i], got[i], float(want[i])) for i in bad[:3]])
    assert all(w == 0 or abs(w) >= Fraction(2) ** -100 for w in want), label       # no subnormal result was asked for


def test_fmaf_is_the_rational_sum_rounded_once_on_20000_triples():
    rng = np.random.default_rng(20241021)
    _assert_exact(*chain_triples(rng, 9000), "chain")
    _assert_exact(*cancelling_triples(rng, 5000), "cancelling")
    _assert_exact(*scaled_triples(rng, 3000), "scaled")
    a, b, c, _side, _m = tie_triples(rng, 3000)
    _assert_exact(a, b, c, "ties")


def test_constructed_ties_land_where_they_should_and_the_naive_form_misses_them():
    rng = np.random.default_rng(7)
    a, b, c, side, m = tie_triples(rng, 3000)
    for s in (-1, 0, 1):
        assert (side == s).sum() > 500
    exact = [Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)) for x, y, z in zip(a, b, c)]
    h = [Fraction(2 * int(mm) + 1, 2 ** 24) for mm in m]
    for e, hh, s in zip(exact, h, side):
        assert (e == hh) if s == 0 else (0 < (e - hh) * int(s) <= Fraction(1, 2 ** 54))
    got = fx.fmaf(a, b, c).astype(np.float64) * 2.0 ** 23                           # in fp32 ulps of [1, 2): m or m + 1
    want = np.where(side == 0, m + (m & 1), np.where(side == 1, m + 1, m))          # the tie to even, else towards the side
    assert np.array_equal(got, want.astype(np.float64))
    naive = naive_fmaf(a, b, c).astype(np.float64) * 2.0 ** 23
    wrong = naive != want
    assert np.array_equal(wrong, ((side == -1) & (m & 1 == 1)) | ((side == 1) & (m & 1 == 0)))
    assert wrong.sum() > 500                                                        # two roundings miss half of the near-ties


def test_fma_fp64_is_the_rational_sum_rounded_once():
    rng = np.random.default_rng(5)
    n = 4000
    a, b = rng.uniform(-20.0, 20.0, n), rng.uniform(-300.0, 300.0, n)
    c = np.concatenate([rng.uniform(-1e3, 1e3, n // 2), -(a * b)[n // 2:]])          # half of them cancel to the product's error
    got = fx.fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        assert Fraction(float(g)) == round_fraction(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)), 53), (x, y, z, g)
    assert fx.fma(3.0, 4.0, 5.0).shape == () and float(fx.fma(3.0, 4.0, 5.0)) == 17.0
