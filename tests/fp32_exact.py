"""Correctly rounded fused multiply-adds on NumPy arrays (not a test module).

NumPy has no fma, and `float32(float64(a) * b + c)` rounds twice: the fp64 sum may land exactly on an fp32 halfway point that the true
sum only comes near, and the cast then breaks a tie that is none.  Both functions here round ONCE:

  fmaf(a, b, c)   fp32.  The product of two fp32 values has 48 bits and is exact in fp64.  c is added with a TwoSum (Knuth), which
                  yields the fp64 sum s and its exact error.  Where the error is not zero and s is even in its last bit, s moves one
                  fp64 ulp towards the error: round to odd.  An odd 53-bit value is never an fp32 halfway point nor an fp32 number, so
                  the cast to fp32 (round to nearest even) of it rounds as it would round the exact sum (53 >= 24 + 2 bits).
  fma(a, b, c)    fp64, by Boldo and Melquiond's emulation ("Emulation of a FMA and correctly rounded sums", 2008): the product as an
                  unevaluated pair by Veltkamp's split and Dekker's product, two TwoSums, the two low parts added with round to odd,
                  then one ordinary addition.

Out of scope, and not checked: results that are fp32 subnormals (the double rounding argument needs the full 24 bits), fp64 products
that overflow, underflow or lose bits to subnormals, NaN and infinities.  The sign of a zero result is whatever the last addition gives.
tests/test_fp32_exact_cpu.py holds both against rational arithmetic.
"""
import numpy as np

_SPLIT = 134217729.0          # 2^27 + 1: Veltkamp's constant for fp64


def two_sum(a, b):
    """(s, e) with s = fl(a + b) and a + b = s + e exactly (Knuth; no condition on the magnitudes)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def add_round_odd(a, b):
    """a + b in fp64 rounded to odd: the exact sum if it is an fp64 value, else the neighbour of it whose last bit is 1."""
    s, e = two_sum(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    s, e = np.atleast_1d(s).copy(), np.atleast_1d(e)
    move = (e != 0.0) & ((s.view(np.int64) & 1) == 0)
    s[move] = np.nextafter(s[move], np.where(e[move] > 0.0, np.inf, -np.inf))
    return s


def fmaf(a, b, c):
    """fl32(a b + c) with one rounding, on float32 arrays (broadcast against each other); returns float32."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    shape = a.shape
    return add_round_odd(a * b, c).astype(np.float32).reshape(shape)


def _split(a):
    t = _SPLIT * a
    hi = t - (t - a)
    return hi, a - hi


def two_prod(a, b):
    """(p, e) with p = fl(a b) and a b = p + e exactly (Dekker), on fp64 arrays away from overflow and underflow."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """fl64(a b + c) with one rounding, on float64 arrays (broadcast against each other)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a, b, c)))
    shape = a.shape
    uh, ul = two_prod(a, b)
    th, tl = two_sum(c, ul)
    vh, vl = two_sum(uh, th)
    return (vh + add_round_odd(tl, vl).reshape(shape)).reshape(shape)
