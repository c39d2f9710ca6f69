"""The one-sine pair sum of the European path kernels (olmc_kernels.h, "Pair sums"), checked without a GPU.

A kernel that needs only the sum of a Box-Muller pair forms rad * sin(turns + 1/8) instead of rad * (cos + sin): the eighth
of a turn is an integer add of 2^20 to the angle word before its 23-bit mantissa mask.  These tests pin the exactness of that
rotation over the whole angle lattice, the identity it rests on, the scale constants, and the compiled loop's instruction mix."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optionslab_amd", "csrc")
EIGHTH_TURN = 0x00100000
MANT = 0x007FFFFF
ONE = 0x3F800000


def _header_constant(path, name):
    with open(os.path.join(CSRC, path)) as f:
        m = re.search(rf"\b{name}\s*=\s*([0-9.eE+-]+)f?\s*;", f.read())
    assert m, name
    return float(m.group(1))


def _turns(words: np.ndarray) -> np.ndarray:
    """The device's angle float of a (shifted) word: the low 23 bits as the mantissa of a float in [1, 2)."""
    return ((words & MANT) | ONE).view(np.float32)


def test_header_carries_the_shift_of_an_eighth_turn():
    with open(os.path.join(CSRC, "olmc_kernels.h")) as f:
        src = f.read()
    assert re.search(r"kEighthTurn\s*=\s*0x00100000u", src)
    assert EIGHTH_TURN * 8 == MANT + 1


def test_shifted_angle_is_exactly_the_rotated_lattice_point_for_every_mantissa():
    m = np.arange(1 << 23, dtype=np.uint32)
    want = (1.0 + np.mod(m.astype(np.float64) * 2.0**-23 + 0.125, 1.0)).astype(np.float32)   # exact: every value is on the lattice
    assert np.array_equal(_turns(m + np.uint32(EIGHTH_TURN)), want)
    # the word's upper nine bits (the add may carry into them or wrap past 2^32) never reach the angle
    for hi in (0x00800000, 0x5A000000, 0xFF800000):
        assert np.array_equal(_turns(m | np.uint32(hi)), _turns(m))
        assert np.array_equal(_turns((m | np.uint32(hi)) + np.uint32(EIGHTH_TURN)), want)


def test_rotation_is_a_permutation_of_the_angle_lattice():
    m = np.arange(1 << 23, dtype=np.uint32)
    shifted = ((m + np.uint32(EIGHTH_TURN)) & MANT)
    assert np.array_equal(np.sort(shifted), m)         # every pair sum keeps its distribution exactly


def test_cos_plus_sin_is_sqrt2_sin_of_the_shifted_angle_on_the_lattice():
    m = np.arange(1 << 23, dtype=np.uint32)
    theta = 2.0 * np.pi * (m.astype(np.float64) * 2.0**-23)
    # the device's periodic sine takes revolutions: the float in [1, 2) minus one whole turn is the angle
    shifted = 2.0 * np.pi * (_turns(m + np.uint32(EIGHTH_TURN)).astype(np.float64) - 1.0)
    err = np.abs((np.cos(theta) + np.sin(theta)) - np.sqrt(2.0) * np.sin(shifted))
    assert err.max() < 4e-15


def test_scale_constants():
    z_scale = _header_constant("olmc_host_math.h", "kZScale")
    pair = _header_constant("olmc_host_math.h", "kPairZScale")
    assert z_scale == pytest.approx(np.sqrt(2.0 * np.log(2.0)), rel=1e-16, abs=0)
    assert pair == pytest.approx(2.0 * np.sqrt(np.log(2.0)), rel=1e-16, abs=0)
    assert pair == pytest.approx(z_scale * np.sqrt(2.0), rel=2e-16, abs=0)
    assert np.float32(_header_constant("olmc_kernels.h", "kInvSqrt2F")) == np.float32(1.0 / np.sqrt(2.0))
    assert _header_constant("olmc_kernels.h", "kSqrt2") == np.sqrt(2.0)


@pytest.mark.parametrize("key", ["c2_european", "c3_fused8", "c3_fused14"])
def test_isa_mix_loop_has_one_sine_per_pair_and_no_cosine(key):
    with open(os.path.join(ROOT, "optionslab_amd", "isa_mix.json")) as f:
        loop = json.load(f)[key]
    ops = loop["by_mnemonic"]
    assert loop["steps_per_trip"] == 16
    assert "v_cos_f32" not in ops
    assert ops.get("v_sin_f32") == 8 and ops.get("v_log_f32") == 8 and ops.get("v_sqrt_f32") == 8
