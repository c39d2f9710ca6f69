"""CPU checks of tests/reduction_reference.py, the plain reference of the synthetic values olmc_reduce_probe reduces on the device:
the vectorised hashes against a scalar restatement, the separable closed form against the brute-force sum over every thread, and the
exactness budget (every total of the shapes tests/test_gpu_reduction.py launches stays below 2^53)."""
import math

import numpy as np
import pytest

from tests import reduction_reference as ref

SALTS = (0, 1, 42, 0xFFFFFFFF, 0x1_0000_0000, 0x1234_5678_9ABC_DEF0, 2 ** 64 - 1)


def test_vectorised_hashes_equal_the_scalar_restatement():
    rng = np.random.default_rng(11)
    bs = [0, 1, 255, 256, 65_536, 65_537, ref.MAX_WORKGROUPS - 1] + [int(x) for x in rng.integers(0, ref.MAX_WORKGROUPS, 40)]
    ts = [0, 1, 31, 32, 63, 64, 255] + [int(x) for x in rng.integers(0, ref.BLOCK, 40)]
    cs = [0, 1, 4, 7, 15, 31] + [int(x) for x in rng.integers(0, 32, 41)]
    checked = 0
    for salt in SALTS:
        assert int(ref.seed32(salt)) == ref.seed32_scalar(salt)
        h = ref.hash_h(np.array(bs, dtype=np.uint64), np.array(cs, dtype=np.uint64), salt)
        k = ref.hash_k(np.array(ts, dtype=np.uint64), np.array(cs, dtype=np.uint64), salt)
        for i, (b, t, c) in enumerate(zip(bs, ts, cs)):
            hs, ks = ref.hash_h_scalar(b, c, salt), ref.hash_k_scalar(t, c, salt)
            assert (int(h[i]), int(k[i])) == (hs, ks), (b, t, c, salt)
            assert hs & 1 and ks & 1 and hs < 2 ** 24 and ks < 2 ** 16
            checked += 1
    assert checked >= 300
    # the hashes do depend on each of their arguments, the upper word of the salt included
    assert ref.hash_h_scalar(5, 3, 1) != ref.hash_h_scalar(5, 3, 1 + 2 ** 32) != ref.hash_h_scalar(6, 3, 1 + 2 ** 32)
    assert ref.hash_k_scalar(5, 3, 1) != ref.hash_k_scalar(5, 4, 1) != ref.hash_k_scalar(6, 4, 1)


@pytest.mark.parametrize("n_threads", [1, 2, 255, 256, 257, 511, 512, 513, 1000, 256 * 33 - 255, 256 * 65 - 1, 256 * 257])
def test_separable_closed_form_equals_the_sum_over_every_thread(n_threads):
    for nv, salt in ((2, 7), (5, 2 ** 40 + 3), (32, 99), (39, 2 ** 33 + 5)):
        v = ref.thread_values(nv, n_threads, salt)
        assert v.shape == (n_threads, nv)
        brute = [sum(int(x) for x in v[:, c]) for c in range(nv)]
        assert ref.expected(nv, n_threads, salt) == brute
        # and one thread at a time, from the scalar hashes
        i = n_threads - 1
        assert [int(x) for x in v[i]] == [ref.hash_h_scalar(i // 256, c, salt) + ref.hash_k_scalar(i % 256, c, salt) for c in range(nv)]


def test_every_total_of_the_gpu_shapes_is_an_exact_double():
    worst = 0
    for nv, form in ref.NV_FORMS:
        for blocking in (0, 1):
            for n, salt in zip(ref.sweep_threads(), ref.sweep_salts(nv, form, blocking)):
                worst = max(worst, max(ref.expected(nv, n, salt)))
    for nv in (2, 5, 32):
        n, salts = ref.sequence(nv)
        assert len(set(salts)) == len(salts) == ref.SEQUENCE_LAUNCHES
        assert [ref.workgroups(x) for x in n[:8]] == list(ref.SEQUENCE_G)
        worst = max(worst, max(max(ref.expected(nv, x, s)) for x, s in zip(n, salts)))
    for nv in (2, 32):
        n, salts = ref.big_launches()
        assert [ref.workgroups(x) for x in n] == [65_537, 65_537, 2 ** 18, 2 ** 18]
        worst = max(worst, max(max(ref.expected(nv, x, s)) for x, s in zip(n, salts)))
    for nv in ref.HAND_OVER_NV:
        n, salts = ref.hand_over_launches(nv)
        assert len(set(salts)) == len(salts) == 3 * len(ref.HAND_OVER_G1) and max(salts) > 2 ** 32
        assert [ref.workgroups(x) for x in n[::3]] == list(ref.HAND_OVER_G1) and max(ref.HAND_OVER_G1) == 1024
        worst = max(worst, max(max(ref.expected(nv, x, s)) for x, s in zip(n, salts)))
    assert worst < 2 ** 53
    assert worst < 2 ** 26 * (2 ** 24 + 2 ** 16) < 2 ** 51         # the budget the tap's header states
    assert float(worst) == worst and float(worst + 1) == worst + 1


def test_the_padded_widths_are_the_kernels_own():
    """NVP, SUBS, kBatch of workgroup_rows_sum / wave_rows_sum and P of block_row_sum, as olmc_kernels.h has them: the Heston American
    fit's 10, 22 and 39 sums pad to 16, 32 and 64, and 64 leaves four row subsets of sixteen loads each."""
    assert [ref.padded_width(nv, True) for nv in (5, 8, 10, 16, 22, 32, 39)] == [8, 8, 16, 16, 32, 32, 64]
    assert [ref.subs_batch(nv, True) for nv in (5, 8, 10, 16, 22, 32, 39)] == [(32, 8), (32, 8), (16, 16), (16, 16), (8, 16), (8, 16), (4, 16)]
    assert [ref.subs_batch(nv, False) for nv in (2, 5)] == [(32, 8), (8, 8)]
    assert [ref.transpose_width(nv) for nv in (2, 5, 8, 10, 16, 22, 32, 39)] == [2, 8, 8, 16, 16, 32, 32, 64]
    assert set(ref.HAND_OVER_NV) == {16, 10, 22, 39} and {nv for nv, _ in ref.NV_FORMS} == {2, 5, 8, 10, 16, 22, 32}
    assert ref.HAND_OVER_G2 == (1, 3, 256)


def test_sweep_salts_differ_and_reach_above_32_bits():
    seen = set()
    for nv, form in ref.NV_FORMS:
        for blocking in (0, 1):
            s = ref.sweep_salts(nv, form, blocking)
            assert len(s) == len(ref.sweep_threads()) == 45 and max(s) > 2 ** 32
            seen.update(s)
    assert len(seen) == 45 * 2 * len(ref.NV_FORMS)


def test_rounded_values_are_the_integers_over_three_and_their_sum_rounds():
    nv, n, salt = 2, 700, 5
    v = ref.rounded_values(nv, n, salt)
    ints = ref.thread_values(nv, n, salt)
    assert all(v[i, c] == int(ints[i, c]) / 3 for i in (0, 1, 255, 256, 699) for c in range(nv))
    fs, sabs, count = ref.rounded_reference(nv, n, salt)
    assert count == n and fs == sabs                                 # all positive
    for c in range(nv):
        exact_thirds = sum(int(x) for x in ints[:, c])                # 3 x the unrounded sum
        assert abs(fs[c] * 3 - exact_thirds) <= n * 2.0 ** -53 * sabs[c] * 3 + 1
        assert math.fsum(v[:, c]) == fs[c]


def test_the_taps_refuse_bad_arguments_before_touching_a_device():
    """OLMC_ERR_ARG (1) with a message, like the other taps; no device is initialised here."""
    import ctypes as C

    from optionslab_amd.build import build_probe_library
    from tools.probe import binding as probe

    build_probe_library()
    lib = probe.hip.load_library()
    n, s, out = (C.c_int64 * 1)(256), (C.c_uint64 * 1)(1), (C.c_double * 40)()
    for args, message in (((3, 0, 0, 1, 1, n, s, out), "nv must be 2, 5, 8, 10, 16, 22 or 32 (39: form 3 only, a workspace row holds 32 values)"),
                          ((39, 0, 0, 1, 1, n, s, out), "nv must be 2, 5, 8, 10, 16, 22 or 32 (39: form 3 only, a workspace row holds 32 values)"),
                          ((2, 1, 0, 1, 1, n, s, out), "form 1 (the folded first exchange) exists for nv 8 and wider"),
                          ((5, 1, 0, 1, 1, n, s, out), "form 1 (the folded first exchange) exists for nv 8 and wider"),
                          ((2, 4, 0, 1, 1, n, s, out), "form must be 0, 1, 2 or 3"),
                          ((2, -1, 0, 1, 1, n, s, out), "form must be 0, 1, 2 or 3"),
                          ((2, 3, 0, 1, 1, n, s, out), "form 3 (the LSM chains' hand-over) exists for nv 10, 16, 22 and 39"),
                          ((32, 3, 0, 0, 1, n, s, out), "form 3 (the LSM chains' hand-over) exists for nv 10, 16, 22 and 39"),
                          ((39, 3, 0, 0, 1, (C.c_int64 * 1)(0), s, out), "n_threads must be >= 1"),
                          ((39, 3, 0, 0, 1, (C.c_int64 * 1)(256 * 1024 + 1), s, out), "form 3 takes at most 1024 workgroups in its first launch"),
                          ((39, 3, 0, 0, 0, n, s, out), "launches must be in [1, 4096]"),
                          ((39, 3, 0, 0, 4097, n, s, out), "launches must be in [1, 4096]"),
                          ((39, 3, 0, 0, 1, None, s, out), "null pointer"),
                          ((2, 0, 0, 1, 0, n, s, out), "launches must be in [1, 4096]"),
                          ((2, 0, 0, 1, 1, None, s, out), "null pointer"),
                          ((2, 0, 0, 1, 1, n, s, None), "null pointer"),
                          ((2, 0, 0, 1, 1, (C.c_int64 * 1)(0), s, out), "n_threads must be >= 1"),
                          ((2, 0, 0, 1, 1, (C.c_int64 * 1)((1 << 26) + 1), s, out), "n_threads beyond one launch of 2^18 workgroups")):
        assert lib.olmc_reduce_probe(*args) == 1
        assert lib.olmc_last_error().decode() == message
    rows = (C.c_double * 64)()
    assert lib.olmc_rows_sum_probe(8, 0, rows, 2, out) == 1 and lib.olmc_rows_sum_probe(2, 1, rows, 2, out) == 1
    assert lib.olmc_rows_sum_probe(2, 0, rows, 0, out) == 1 and lib.olmc_rows_sum_probe(2, 0, None, 2, out) == 1
    for nv, whole in ((10, 0), (22, 0), (39, 0), (64, 1), (40, 1), (11, 1)):
        assert lib.olmc_rows_sum_probe(nv, whole, rows, 1, out) == 1
        assert lib.olmc_last_error().decode() == "nv must be 2 or 5 for one wave, 5, 8, 10, 16, 22, 32 or 39 for the whole workgroup"
    assert lib.olmc_wave_reduce_probe(3, 0, rows, out) == 1 and lib.olmc_wave_reduce_probe(2, 3, rows, out) == 1
    assert lib.olmc_wave_reduce_probe(2, 0, None, out) == 1
    for p in (0, 48, 128):
        assert lib.olmc_wave_reduce_probe(p, 0, rows, out) == 1 and lib.olmc_last_error().decode() == "p must be 1, 2, 4, 8, 16, 32 or 64"
    # the two taps of the in-wave solvers
    totals, beta, valid = (C.c_double * 64)(), (C.c_double * 16)(), (C.c_int32 * 1)()
    for entry, top in ((lib.olmc_ha_fit_probe, 3), (lib.olmc_lsm_fit_probe, 4)):
        for args, message in (((0, totals, 1, beta, valid), f"degree must be in [1, {top}]"),
                              ((top + 1, totals, 1, beta, valid), f"degree must be in [1, {top}]"),
                              ((1, None, 1, beta, valid), "null pointer"), ((1, totals, 1, None, valid), "null pointer"),
                              ((1, totals, 1, beta, None), "null pointer"),
                              ((1, totals, 0, beta, valid), "n_sets must be in [1, 4096]"), ((1, totals, 4097, beta, valid), "n_sets must be in [1, 4096]")):
            assert entry(*args) == 1
            assert lib.olmc_last_error().decode() == message
