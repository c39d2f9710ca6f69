"""CPU checks of tests/box_muller_reference.py, the plain NumPy reference the GPU tests of the device's Box-Muller transform
(tests/test_gpu_box_muller.py) are gated against: its Philox against Random123's known answer and the C checker's, its transform
against the C checker's, the properties of the specification the GPU tests rely on, and the fixture of extreme draws."""
import json
import math
import os

import numpy as np
import pytest

from oracle import philox_oracle as po
from tests import box_muller_reference as bm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extreme_draws.json")


def test_numpy_philox_reproduces_the_random123_known_answers():
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = bm.philox4x32_10(*(np.array([c]) for c in ctr), *key)
        assert tuple(int(g[0]) for g in got) == want


@pytest.mark.parametrize("seed,path0,block,tag", [(42, 0, 0, 0), (7, 123_456, 3, 0), (2 ** 63 + 5, (1 << 32) - 50, 62, 1),
                                                  (0xDEADBEEFCAFE, (1 << 40) + 17, 1, 2)])
def test_numpy_philox_matches_the_checkers_words(seed, path0, block, tag):
    """100 consecutive paths per case: around 0, across 2^32 (the path's high word becomes 1 mid-way), above 2^40, a seed with a high
    key word, non-zero blocks and stream tags."""
    want = po.philox_words(seed, path0, 100, block, 1, tag)[:, 0, :]
    got = bm.philox_words(seed, path0 + np.arange(100, dtype=np.uint64), block, tag)
    assert got.dtype == np.uint32 and np.array_equal(got, want)


def test_numpy_transform_agrees_with_the_checkers():
    """po.normals evaluates the same formulas in fp64 and rounds twice to fp32 (the RAW normal, then its product with fp32(kZScale)):
    2^-22 max(1, |z|) covers both roundings at 2^-24 relative each with a factor two to spare (measured: 1.18e-7)."""
    n_paths, n_steps = 513, 252
    words = po.philox_words(42, 1000, n_paths, 0, n_steps // 4)
    _, c0, s0, _ = bm.raw(words[..., 0], words[..., 1])
    _, c1, s1, _ = bm.raw(words[..., 2], words[..., 3])
    z = bm.Z_SCALE * np.stack([c0, s0, c1, s1], axis=-1).reshape(n_paths, n_steps)
    want = po.normals(42, 1000, n_paths, n_steps).astype(np.float64)
    err = np.abs(z - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 2.0 ** -22, err.max()


def test_pair_is_the_sum_of_the_two_normals_over_sqrt2_on_the_whole_lattice():
    """The eighth-turn identity cos t + sin t = sqrt(2) sin(t + 1/8) on all 2^23 lattice angles, the wrap range included."""
    k = np.arange(1 << 23, dtype=np.uint32)
    _, c, s, pair = bm.raw(np.full(k.size, bm.RAD_ONE_WORD, dtype=np.uint32), k)
    assert np.abs((c + s) / math.sqrt(2.0) - pair).max() <= 1e-15
    quarter = 1 << 21
    assert c[0] == 1.0 and s[0] == 0.0 and c[quarter] == 0.0 and s[quarter] == 1.0 and c[2 * quarter] == -1.0 and s[2 * quarter] == 0.0
    assert c[3 * quarter] == 0.0 and s[3 * quarter] == -1.0 and pair[7 << 20] == 0.0 and pair[3 << 20] == 0.0


def test_properties_of_the_specification_the_gpu_tests_rely_on():
    top = np.arange((1 << 32) - 4096, 1 << 32, dtype=np.int64).astype(np.uint32)
    ua = bm.ua32(top)
    assert ua.dtype == np.float32 and ua.max() == 1.0                                       # never above 1
    assert np.array_equal(top[ua == 1.0], np.arange(bm.ONE_WORDS, 1 << 32, dtype=np.int64).astype(np.uint32)) and (ua == 1.0).sum() == 128
    assert np.all(bm.radius(top[ua == 1.0]) == 0.0)
    everywhere = np.concatenate([bm.radius_edge_words(), bm.radius_strided_words()])
    ua = bm.ua32(everywhere)
    assert ua.min() == np.float32(2.0 ** -33) == bm.ua32(np.array([0], dtype=np.uint32))[0] and ua.max() <= 1.0
    assert np.all(np.diff(bm.ua32(np.sort(everywhere)).astype(np.float64)) >= 0)             # monotone in the word
    rad = bm.radius(everywhere)
    assert rad.max() == bm.radius(np.array([0], dtype=np.uint32))[0] == math.sqrt(33.0)
    assert bm.Z_SCALE * rad.max() == pytest.approx(math.sqrt(2 * 33 * math.log(2)), rel=1e-15)
    assert bm.radius(np.array([bm.RAD_ONE_WORD], dtype=np.uint32))[0] == 1.0                # the angle sweep's radius
    assert float(bm.Z_SCALE_F32) == pytest.approx(bm.Z_SCALE, rel=2.0 ** -24)


def test_chosen_inputs_cover_the_edges_they_name():
    edges, strided = bm.radius_edge_words(), bm.radius_strided_words()
    assert edges.size == 2 * 4096 + 93 and strided.size == 1 << 20 and strided[0] == 2049 and strided[-1] == (1 << 32) - 2047
    for w in (0, 127, 128, 4095, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001, 1 << 24, (1 << 24) + 1):
        assert w in edges
    plain, rnd = bm.angle_words()
    assert rnd.size == 16 and set(plain.tolist()) >= {0, 1, 0x7FFFFF, 0x0FFFFF, 0x100000, 0x100001, 0x6FFFFF, 0x700000, 0x700001, 0x400000}
    s = bm.angle_stratum(np.array([0, 1, 2, 0x7FFFFF, 0x7FFFFE, 0x100000, 0x6FFFFF, 0x700002, 0x123456]))
    assert [bm.ANGLE_STRATA[i] for i in s] == ["lattice_zeros", "lattice_zeros", "bulk", "lattice_zeros", "wrap_range", "lattice_zeros", "lattice_zeros",
                                               "wrap_range", "bulk"]
    r = bm.radius_stratum(np.array([0, 127, 128, 0xFFFFEFFF, 0xFFFFF000, 0xFFFFFFFF], dtype=np.uint32))
    assert [bm.RADIUS_STRATA[i] for i in r] == ["tail_words", "tail_words", "bulk", "bulk", "near_one", "near_one"]


def test_every_fixture_entry_holds_its_word():
    doc = json.load(open(FIXTURE))
    entries = doc["entries"]
    kinds = [e["kind"] for e in entries]
    assert kinds.count("tail") >= 4 and kinds.count("one") >= 4 and {e["seed"] for e in entries} == {42, 7} and doc["block"] == 0
    for e in entries:
        assert e["slot"] in (0, 2) and 0 <= e["path"] < doc["paths_scanned"]
        assert (e["word"] < bm.TAIL_WORDS) if e["kind"] == "tail" else (e["word"] >= bm.ONE_WORDS)
        assert int(po.philox_words(e["seed"], e["path"], 1, 0, 1)[0, 0, e["slot"]]) == e["word"], e
        z = po.normals(e["seed"], e["path"], 1, 4)[0, e["slot"]:e["slot"] + 2].astype(np.float64)
        if e["kind"] == "one":
            assert np.all(z == 0.0)
        else:
            assert math.hypot(*z) > 5.8
    known = {(e["seed"], e["path"]): e for e in entries}
    assert known[(42, 26967075)]["word"] == 0xC and known[(42, 52825872)]["word"] == 0xFFFFFFBE
