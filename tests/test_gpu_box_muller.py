"""The normal generator under every Philox kernel -- box_muller_raw and pair_sum_raw of olmc_kernels.h -- and the Heston kernels'
sqrt_nonneg, on CHOSEN words and edges through the instrumented build's taps (olmc_box_muller_probe, olmc_sqrt_nonneg_probe), against
the plain fp64 reference of tests/box_muller_reference.py; and the product's pricing kernels on paths whose first Philox block holds
such a word (tests/golden/extreme_draws.json).

A seeded stream meets a radius word that rounds u_a to 1, a 6-sigma tail word, a zero of the hardware sine or the wrap of the
eighth-turn shift once in about 2^25 draws, so the few hundred thousand draws of the parity and pair-sum tests never evaluate them.

The gate.  For z_cos, z_sin and pair (RAW units; a true normal is kZScale times the RAW one):

    kZScale |device - reference| <= Z_ABS_TOL max(1, kZScale rad),     Z_ABS_TOL = 2e-5,

the per-normal bound tests/test_gpu_parity.py enforces on typical draws, times the radius where that exceeds one normal unit: the
error of v_sin_f32 / v_cos_f32 is absolute and the radius multiplies it.  Measured worst errors per stratum:
profiles/r12_box_muller_accuracy.jsonl (tools/box_muller_accuracy.py runs the same measuring code through the same tap; every test
here prints its figures before it asserts, visible with -s).  Worst gate ratio measured: 2.1e-7 (bulk radius words), 1.7e-7 on the
tail words, 1.9e-10 next to u_a = 1, 4.8e-8 on the lattice zeros, 1.1e-7 in the wrap range -- a hundredth of the gate everywhere.
"""
import json
import math
import os

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import box_muller_reference as bm
from tests.gpu_support import device_fixture
from tools.probe import binding as probe

pytestmark = pytest.mark.gpu

hip = probe.hip
ENTRIES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extreme_draws.json")))["entries"]
ENTRY_IDS = [f"{e['kind']}-seed{e['seed']}-path{e['path']}-x{e['slot']}" for e in ENTRIES]
S, K, T, R, SIGMA = 100.0, 1.0, 1.0, 0.05, 0.2          # a deep in-the-money call: no payoff clips to zero


_device = device_fixture(hip)


def _assert_gate(measured):
    print(json.dumps(measured["worst"]))
    assert measured["finite"]
    for stratum, outputs in measured["worst"].items():
        for name, w in outputs.items():
            assert w["ratio"] <= bm.Z_ABS_TOL, (stratum, name, w)


# ------------------------------------------------------------------ the tap is the product's code
def test_the_tap_times_kzscale_is_the_normals_tap_bit_for_bit():
    """olmc_normals reports kZScaleF * box_muller_raw(words) of the stream; the tap on the very words of that stream, times the same
    fp32 constant, is the same function's result through the same single multiply: equal bits, in both builds."""
    n_paths, n_steps = 513, 252
    words = _hip.philox_words(42, 1000, n_paths, 0, n_steps // 4)
    c0, s0, _ = probe.box_muller_probe(words[..., 0], words[..., 1])
    c1, s1, _ = probe.box_muller_probe(words[..., 2], words[..., 3])
    got = (bm.Z_SCALE_F32 * np.stack([c0, s0, c1, s1], axis=-1)).reshape(n_paths, n_steps)
    assert got.dtype == np.float32
    want = _hip.normals(42, 1000, n_paths, n_steps)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want.view(np.uint32), hip.normals(42, 1000, n_paths, n_steps).view(np.uint32))


# ------------------------------------------------------------------ chosen words against the fp64 reference
@pytest.fixture(scope="module")
def angle_sweep():
    return bm.measure_angle_sweep(probe.box_muller_probe)


@pytest.fixture(scope="module")
def edge_cross():
    return bm.measure_radius_cross(probe.box_muller_probe, bm.radius_edge_words())


@pytest.fixture(scope="module")
def strided_cross():
    return bm.measure_radius_cross(probe.box_muller_probe, bm.radius_strided_words())


def test_every_lattice_angle_at_unit_radius_meets_the_gate(angle_sweep):
    """All 2^23 mantissas at x_a = 0x80000000 (u_a = 1/2, rad = 1): what v_cos_f32 / v_sin_f32 return on the whole lattice, the zeros
    of the quarter and eighth turns and the mantissas >= 0x700000 where the pair sum's eighth-turn add wraps."""
    assert set(angle_sweep["worst"]) == set(bm.ANGLE_STRATA)
    _assert_gate(angle_sweep)


def test_radius_edges_at_every_chosen_angle_meet_the_gate(edge_cross):
    """0 .. 4095 (|z| up to 6.76: the radius multiplies the sine's error by up to 5.74), the top 4096 words (-log2 u_a down to 8.6e-8:
    the RELATIVE accuracy of v_log_f32 next to 1) and the powers of two +-1 (where (float) x_a changes its rounding), each at the
    lattice angles and 16 random words."""
    assert set(edge_cross["worst"]) == set(bm.RADIUS_STRATA) and edge_cross["n"] == (2 * 4096 + 93) * (bm.angle_words()[0].size + 16)
    _assert_gate(edge_cross)


def test_radius_words_across_the_range_at_every_chosen_angle_meet_the_gate(strided_cross):
    """2^20 words 4096 j + 2049 at the same angles: the radius at every 2^-20 of its range."""
    assert strided_cross["n"] == (1 << 20) * (bm.angle_words()[0].size + 16)
    _assert_gate(strided_cross)


def test_a_radius_that_rounds_to_one_gives_exact_zeros_at_every_angle(angle_sweep, edge_cross):
    """x_a >= 0xFFFFFF80: u_a == 1.0f, log2 is an exact 0 and all three outputs are zeros (of either sign), never the NaN of a square
    root of a slightly positive logarithm -- at the chosen angles for all 128 words, on the whole lattice for the last one."""
    assert edge_cross["finite"] and edge_cross["zeros_at_one"]
    assert angle_sweep["zeros_at_one"]


def test_the_upper_nine_bits_of_the_angle_word_never_change_an_output(angle_sweep, edge_cross, strided_cross):
    """Compared by bits: w and w | 0xFF800000, at every lattice mantissa for rad = 1 and at the chosen angles for every radius word
    (the pair sum adds 2^20 BEFORE the mask, so a carry out of the mantissa must vanish in it)."""
    assert angle_sweep["upper_bits_ignored"] and edge_cross["upper_bits_ignored"] and strided_cross["upper_bits_ignored"]


# ------------------------------------------------------------------ sqrt_nonneg
@pytest.fixture(scope="module")
def sqrt_measured():
    m = bm.measure_sqrt(probe.sqrt_nonneg_probe)
    print(json.dumps(m))
    return m


def test_sqrt_nonneg_is_within_one_ulp_where_the_kernels_claim_it(sqrt_measured):
    """olmc_kernels.h: "1 ulp against sqrt over [1e-12, 10]" -- 400,000 log-uniform points against numpy.sqrt (correctly rounded), and
    the exact squares k^2 2^-40, k = 1 .. 4096, whose roots are representable.  Measured: no point differs from numpy.sqrt at all."""
    for name in ("claimed", "squares"):
        m = sqrt_measured[name]
        assert m["finite"] and m["non_negative"] and m["ulp"] <= 1.0, (name, m)


def test_sqrt_nonneg_of_zero_is_zero():
    """Every truncated variance: max(v, 0) = 0 must give a root of exactly 0 (the seed is v_rsq_f32 of the clamp 1e-30f, not of 0)."""
    y = probe.sqrt_nonneg_probe(np.array([0.0, -0.0]))
    assert y[0] == 0.0 and y[1] == 0.0


def test_sqrt_nonneg_beside_the_claimed_range(sqrt_measured):
    """[1e-30, 1e-12) and (10, 1e30]: finite, non-negative, relative error <= 2^-40 -- derived, not measured: the 2^-22 seed squared
    once by the Goldschmidt round leaves (3/2) 2^-44 before the residual correction."""
    for name in ("below", "above"):
        m = sqrt_measured[name]
        assert m["finite"] and m["non_negative"] and m["rel"] <= 2.0 ** -40, (name, m)


def test_sqrt_nonneg_below_1e_30_is_immaterial(sqrt_measured):
    """Below the clamp of the seed the root (< 1e-15) loses accuracy: finite, non-negative and within 1e-15 of sqrt, subnormals
    included."""
    m = sqrt_measured["tiny"]
    assert m["finite"] and m["non_negative"] and m["abs_err"] <= 1e-15, m


@pytest.mark.parametrize("bad", [-1e-300, -1.0, math.nan, math.inf])
def test_sqrt_nonneg_tap_refuses_what_the_kernels_never_hand_it(bad):
    with pytest.raises(ol.AccelerationError):
        probe.sqrt_nonneg_probe(np.array([1.0, bad]))


# ------------------------------------------------------------------ extreme draws through the product
def _bounds(rad):
    """Per-normal gate bounds of one path's steps; a step whose radius is an exact zero must be an exact zero on the device."""
    return np.where(rad == 0.0, 0.0, bm.gate(rad))


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_extreme_draw_normals_meet_the_gate_and_equal_the_tap(entry):
    seed, path, slot = entry["seed"], entry["path"], entry["slot"]
    words = _hip.philox_words(seed, path, 1, 0, 1)[0, 0]
    assert int(words[slot]) == entry["word"]
    z = _hip.normals(seed, path, 1, 4)[0]
    want, rad = bm.path_normals(seed, path, 4)
    assert np.isfinite(z).all() and (np.abs(z - want) <= _bounds(rad)).all(), (z, want)
    c, s, _ = probe.box_muller_probe(words[[0, 2]], words[[1, 3]])
    tap = bm.Z_SCALE_F32 * np.array([c[0], s[0], c[1], s[1]], dtype=np.float32)
    assert np.array_equal(tap.view(np.uint32), z.view(np.uint32))
    pair = z[slot:slot + 2].astype(np.float64)
    if entry["kind"] == "one":
        assert (pair == 0.0).all() and (want[slot:slot + 2] == 0.0).all()
    else:
        assert math.hypot(*pair) > 5.8


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_extreme_draw_prices_one_path_at_a_time(entry):
    """n_paths = 1, antithetic off, path_offset = the path: st.sum is that path's payoff.  olmc_european with 1, 2, 3 and 4 steps
    (the odd leftover cosine; one pair sum; pair + cosine; the full block), the arithmetic Asian at the reference's precision and the
    fixed-strike lookback with 4 steps (box_muller_raw inside a per-date kernel), against the payoff rebuilt in fp64 from the reference
    normals.  Relative tolerance: an error dz of a normal moves ln S by vol dz, so vol * (sum of the per-normal gate bounds of the steps
    used) + 1e-12 -- for a path of exact zeros, 1e-12 alone."""
    seed, path = entry["seed"], entry["path"]
    z4, rad4 = bm.path_normals(seed, path, 4)

    def rel_tol(m):
        return SIGMA * math.sqrt(T / m) * _bounds(rad4[:m]).sum() + 1e-12

    for m in (1, 2, 3, 4):
        st = _hip.european(S, K, T, R, SIGMA, 0.0, True, 1, m, seed, False, path_offset=path)
        want = bm.gbm_spots(z4[:m], S, T, R, SIGMA)[-1] - K
        assert st.n == 1 and math.isfinite(st.sum) and abs(st.sum - want) <= rel_tol(m) * want, (m, st.sum, want)
    spots = bm.gbm_spots(z4, S, T, R, SIGMA)
    asian = _hip.asian(S, K, T, R, SIGMA, 0.0, True, False, 1, 4, seed, False, path_offset=path)
    want = spots.mean() - K
    assert asian.n == 1 and math.isfinite(asian.sum) and abs(asian.sum - want) <= rel_tol(4) * want, (asian.sum, want)
    look = _hip.lookback(S, K, T, R, SIGMA, 0.0, True, True, 1, 4, seed, False, path_offset=path)
    want = max(S, spots.max()) - K
    assert look.n == 1 and math.isfinite(look.sum) and abs(look.sum - want) <= rel_tol(4) * want, (look.sum, want)
    if entry["kind"] == "one":
        m = entry["slot"] + 2                             # the steps up to and including the two exact zeros
        assert (z4[m - 2:m] == 0.0).all()
        st = _hip.european(S, K, T, R, SIGMA, 0.0, True, 1, m, seed, False, path_offset=path)
        want = bm.gbm_spots(z4[:m], S, T, R, SIGMA)[-1] - K
        assert math.isfinite(st.sum) and abs(st.sum - want) <= rel_tol(m) * want
        if m == 2:
            assert want == pytest.approx(S * math.exp((R - 0.5 * SIGMA * SIGMA) * T) - K, rel=1e-15)
