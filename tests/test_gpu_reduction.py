"""The fused grid reduction of olmc_kernels.h (wave_transpose_reduce, block_then_grid_reduce[_from], block_row_sum, grid_reduce,
grid_reduce_workgroup, wave_rows_sum, workgroup_rows_sum) pinned to EXACT sums through the three taps of the instrumented build
(include/olmc_probe.h: olmc_reduce_probe, olmc_rows_sum_probe, olmc_wave_reduce_probe).

Every price, Greek and moment of the library leaves the device through this code, and a pricing test cannot see it fail: one lost
lane in a million paths is 1e-6 of a sum the same-stream ties compare at 2e-6.  A reduction has an exact answer, though.  The taps
feed it integers whose every partial sum fits in 53 bits (tests/reduction_reference.py), so the fp64 result is exact in any order
and must EQUAL a Python integer: a dropped, doubled, stale or misrouted value fails `==`, at every row width (NV 2, 5, 8, 16, 32, and
the Heston American fit's 10, 22 and 39 with their P = 64 transpose and NVP = 64 row sum), entry form -- the LSM chains' two-launch
hand-over among them -- group count and ragged tail the product reaches.  No tolerance anywhere except in the one test of rounded sums, whose
bound is the textbook one for recursive summation in any order."""
import functools
import math
import threading

import numpy as np
import pytest

from tests import reduction_reference as ref
from tests.gpu_support import device_fixture
from tools.probe import binding as probe

pytestmark = pytest.mark.gpu

ATM = (100.0, 100.0, 1.0, 0.05, 0.2)
hip = probe.hip


_device = device_fixture(hip, after=lambda: probe.tune(probe.TUNE_FORCE_NV, 0))


@functools.lru_cache(maxsize=None)
def expected(nv, n_threads, salt):
    return tuple(ref.expected(nv, n_threads, salt))


def assert_exact(out, nv, n_threads, salts, what):
    """Every launch's nv totals EQUAL the reference's integers, and its tail is its n_threads."""
    assert out.shape == (len(n_threads), nv + 1), what
    assert np.isfinite(out).all(), (what, "a total that is not finite", np.argwhere(~np.isfinite(out))[:4].tolist())
    for j, (n, salt) in enumerate(zip(n_threads, salts)):
        got, want = tuple(int(x) for x in out[j, :nv]), expected(nv, n, salt)
        assert all(float(g) == x for g, x in zip(got, out[j, :nv])), (what, j, "a total that is not an integer")
        assert got == want, (what, f"launch {j}: n_threads {n} ({ref.workgroups(n)} workgroups), salt {salt:#x}",
                             [(c, g - w) for c, (g, w) in enumerate(zip(got, want)) if g != w][:4])
        assert int(out[j, nv]) == n, (what, j, "tail", out[j, nv])


# ------------------------------------------------------------------ shape sweep
@pytest.mark.parametrize("blocking", [1, 0], ids=["blocking", "queued"])
@pytest.mark.parametrize("nv,form", ref.NV_FORMS)
def test_every_width_form_and_group_count_sums_exactly(nv, form, blocking):
    """45 launches per case: G in SWEEP_G workgroups -- one group, a group of exactly 256, a second group of one workgroup, the SUBS
    and SUBS * kBatch boundaries of every padded row width -- each full, with a single live thread in the last workgroup and with one
    thread missing."""
    n, salts = ref.sweep_threads(), ref.sweep_salts(nv, form, blocking)
    out = probe.reduce_probe(nv, form, n, salts, values=0, blocking=bool(blocking))
    assert_exact(out, nv, n, salts, (nv, form, blocking))


@pytest.mark.parametrize("blocking", [1, 0], ids=["blocking", "queued"])
@pytest.mark.parametrize("nv", [2, 32])
def test_grids_past_65536_workgroups_sum_exactly(nv, blocking):
    """65,537 workgroups = 257 groups: the second loop trip of the level-2 row sum (one wave for nv = 2, the workgroup for nv = 32);
    2^18 workgroups = 1,024 groups: the largest grid.  Each full and with one live thread in the last workgroup."""
    n, salts = ref.big_launches()
    out = probe.reduce_probe(nv, 0, n, salts, values=0, blocking=bool(blocking))
    assert_exact(out, nv, n, salts, (nv, "big", blocking))


# ------------------------------------------------------------------ back-to-back launches with changing contents
SEQUENCE_REPEATS = 50


@pytest.mark.parametrize("nv", [2, 5, 32])
def test_back_to_back_launches_with_changing_contents_are_each_exact(nv):
    """64 launches queued on one stream with no host wait between them, every one with another salt and the grid cycling through 700,
    1, 257, 256, 1000, 3, 513 and 65,537 workgroups: the same block_rows, group_rows and counters with other contents and other grid
    sizes each time.  A row left over from the launch before has other bits here, and a counter a finisher did not re-zero (or
    re-zeroed without having consumed it) ends the next launch early or never: all 64 results exact, 50 times over."""
    n, salts = ref.sequence(nv)
    for rep in range(SEQUENCE_REPEATS):
        out = probe.reduce_probe(nv, 0, n, salts, values=0, blocking=False)
        assert_exact(out, nv, n, salts, (nv, "sequence", rep))


LOAD_REPEATS = 150         # fixed: about a second of queued launches beside the load threads


@pytest.mark.parametrize("nv", [2, 32])
def test_back_to_back_launches_are_exact_under_load(nv):
    """The same 64-launch sequence while three threads price Europeans of other sizes on three other contexts of the device (in the
    style of test_gpu_parity's one-seed-under-load test): every result exact, every load thread self-consistent."""
    stop, errs, rounds = threading.Event(), [], [0, 0, 0]

    def load(k):
        try:
            N, M = [(10_000, 50), (300_001, 7), (1_000_000, 16)][k]
            first = None
            while not stop.is_set():
                st = hip.european(*ATM, 0.0, True, N, M, 1000 + k, True)
                first = first or (st.sum, st.sumsq)
                if (st.sum, st.sumsq) != first:
                    raise AssertionError(f"load thread {k}: other bits on a repeat")
                rounds[k] += 1
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    n, salts = ref.sequence(nv)
    [expected(nv, x, s) for x, s in zip(n, salts)]          # the reference before the clock of the load threads starts
    ts = [threading.Thread(target=load, args=(k,)) for k in range(3)]
    [t.start() for t in ts]
    try:
        for rep in range(LOAD_REPEATS):
            out = probe.reduce_probe(nv, 0, n, salts, values=0, blocking=False)
            assert_exact(out, nv, n, salts, (nv, "under load", rep))
    finally:
        stop.set()
        [t.join() for t in ts]
    assert not errs, errs[:2]
    assert all(r > 0 for r in rounds), rounds


# ------------------------------------------------------------------ row summers
def _subs_batch(nv, whole_workgroup):
    """(SUBS, kBatch) of wave_rows_sum<nv> / workgroup_rows_sum<nv>: row subsets per column and loads in flight per lane (NVP = 64, the 39
    sums of degree 3: 4 subsets of 16 loads)."""
    return ref.subs_batch(nv, whole_workgroup)


ROW_SUMMERS = [(2, False), (5, False), (5, True), (8, True), (10, True), (16, True), (22, True), (32, True), (39, True)]


@functools.lru_cache(maxsize=None)
def _integer_rows():
    m = np.random.default_rng(7).integers(1, 2 ** 30, size=(1 << 18, 39), dtype=np.int64)
    return m, m.astype(np.float64)


def _row_counts(nv, whole_workgroup):
    s, b = _subs_batch(nv, whole_workgroup)
    return sorted({1, s - 1, s, s + 1, s * b - 1, s * b, s * b + 1, 2 * s * b - 1, 2 * s * b, 2 * s * b + 3, 3 * s * b + 1, 1024, 1025, 65_537, 1 << 18} - {0})


@pytest.mark.parametrize("nv,whole_workgroup", ROW_SUMMERS, ids=[f"{'workgroup' if w else 'wave'}-{nv}" for nv, w in ROW_SUMMERS])
def test_row_summers_sum_every_row_once(nv, whole_workgroup):
    """wave_rows_sum / workgroup_rows_sum on integer matrices at the row counts where their loops change shape (one row, a lane subset
    more or less, a batch of loads more or less, a second trip, 65,537 and 2^18 rows: counts no cheap grid reaches, and the callers that
    hand them gridDim.x rows).  Integers below 2^30 in at most 2^18 rows: every partial sum below 2^48, exact."""
    ints, dbls = _integer_rows()
    for rows in _row_counts(nv, whole_workgroup):
        got = probe.rows_sum_probe(dbls[:rows, :nv], whole_workgroup)
        want = [int(x) for x in ints[:rows, :nv].sum(axis=0)]
        assert np.isfinite(got).all(), (rows, got)
        assert [int(x) for x in got] == want, (nv, whole_workgroup, rows, [int(g) - w for g, w in zip(got, want)])


@pytest.mark.parametrize("nv,whole_workgroup", ROW_SUMMERS, ids=[f"{'workgroup' if w else 'wave'}-{nv}" for nv, w in ROW_SUMMERS])
def test_row_summers_carry_a_nan_and_an_inf_to_their_column_only(nv, whole_workgroup):
    """One NaN in the last row, one inf in row SUBS * kBatch (the first row of a lane's second batch): the column that holds it must
    answer NaN / inf -- one that dropped that row would come out finite -- and every other column stays exact."""
    ints, dbls = _integer_rows()
    s, b = _subs_batch(nv, whole_workgroup)
    rows = 2 * s * b + 3
    want = [int(x) for x in ints[:rows, :nv].sum(axis=0)]
    for row, col, poison in ((rows - 1, nv - 1, math.nan), (s * b, 0, math.inf), (s * b, nv - 1, -math.inf), (rows - 1, 0, math.nan)):
        m = dbls[:rows, :nv].copy()
        m[row, col] = poison
        got = probe.rows_sum_probe(m, whole_workgroup)
        assert (math.isnan(got[col]) if math.isnan(poison) else got[col] == poison), (row, col, poison, got[col])
        others = [c for c in range(nv) if c != col]
        assert np.isfinite(got[others]).all()
        assert [int(got[c]) for c in others] == [want[c] for c in others], (row, col, poison)


# ------------------------------------------------------------------ transpose-reduce
NUMPY_OPS = {"sum": np.sum, "max": np.max, "min": np.min}


def _placed(per_value, p):
    """Lane l holds the result of value index l >> (6 - log2 p) (the contract of wave_transpose_reduce's header comment)."""
    shift = 6 - int(math.log2(p))
    return np.array([per_value[lane >> shift] for lane in range(64)])


@pytest.mark.parametrize("op", ["sum", "max", "min"])
@pytest.mark.parametrize("p", [1, 2, 4, 8, 16, 32, 64])
def test_wave_transpose_reduce_places_every_value_index_on_its_lanes(p, op):
    rng = np.random.default_rng(100 * p + len(op))
    # integers: exact whatever the order of the exchanges
    v = rng.integers(-2 ** 40, 2 ** 40, size=(64, p)).astype(np.float64)
    got = probe.wave_reduce_probe(v, op)
    want = _placed(NUMPY_OPS[op](v, axis=0), p)
    assert np.array_equal(got, want), (p, op, np.argwhere(got != want)[:4].tolist())
    # signed zeros and infinities (an inf of each sign in one column of a sum is a NaN there, in any order)
    z = rng.integers(-3, 4, size=(64, p)).astype(np.float64)
    z[rng.random((64, p)) < 0.3] = -0.0
    z[rng.random((64, p)) < 0.2] = 0.0
    z[5, 0] = math.inf
    z[37, p - 1] = math.inf if (op == "sum" and p == 1) else -math.inf
    if p >= 4:
        z[0, 1], z[63, 1] = math.inf, -math.inf
        z[:, 2] = -0.0
    got = probe.wave_reduce_probe(z, op)
    with np.errstate(invalid="ignore"):
        want = _placed(NUMPY_OPS[op](z, axis=0), p)
    assert np.array_equal(got, want, equal_nan=True), (p, op, got, want)
    if op == "sum" and p >= 4:
        assert math.isnan(got[1 << (6 - int(math.log2(p)))])          # value index 1: inf - inf
    if op != "sum":
        # the extreme in lane 0, 31, 32, 63 (either side of both permlane swaps) and at value index 0 and p - 1 in turn
        base = rng.integers(-1000, 1000, size=(64, p)).astype(np.float64)
        extreme = 1e6 if op == "max" else -1e6
        for lane in (0, 31, 32, 63):
            for index in sorted({0, p - 1}):
                m = base.copy()
                m[lane, index] = extreme
                got = probe.wave_reduce_probe(m, op)
                want = _placed(NUMPY_OPS[op](m, axis=0), p)
                assert want[index << (6 - int(math.log2(p)))] == extreme
                assert np.array_equal(got, want), (p, op, lane, index)


# ------------------------------------------------------------------ rounded sums
@pytest.mark.parametrize("g", [257, 1000])
@pytest.mark.parametrize("nv", [2, 16])
def test_rounded_sums_stay_within_the_bound_of_recursive_summation(nv, g):
    """values = 1: each thread's integer over 3.0, so the additions round.  Whatever the order, recursive summation of n addends errs
    by at most n 2^-53 sum |v| (to first order; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2): a derived
    bound, nothing measured.  The reference is the correctly rounded sum (math.fsum) of the very doubles the threads hold."""
    n = 256 * g - 3
    salt = 0x7_0000_0000 + g
    fs, sabs, count = ref.rounded_reference(nv, n, salt)
    for form in (f for w, f in ref.NV_FORMS if w == nv):
        for blocking in (True, False):
            out = probe.reduce_probe(nv, form, [n], [salt], values=1, blocking=blocking)
            assert int(out[0, nv]) == n
            for c in range(nv):
                err, bound = abs(out[0, c] - fs[c]), count * 2.0 ** -53 * sabs[c]
                print(f"nv {nv} G {g} form {form} blocking {blocking} c {c}: |dev - fsum| {err:.3e} bound {bound:.3e}")
                assert err <= bound, (nv, g, form, blocking, c, out[0, c], fs[c])


@pytest.mark.parametrize("blocking", [True, False], ids=["blocking", "queued"])
@pytest.mark.parametrize("nv", [2, 16])
def test_a_rounded_sum_keeps_its_bits_between_neighbours_that_change(nv, blocking):
    """`price1 == price2` with a neighbour that changes: the same rounded launch 200 times, each followed by a launch of another
    salt and size on the same workspace -- ONE distinct set of bits (sums run in index order, never arrival order)."""
    n0, salt0 = 256 * 1000 - 3, 0x7_0000_0000 + 1000
    sizes = [256 * g - r for g in (1, 3, 257, 700, 256, 513, 1000, 65) for r in (0, 9)]
    n = [x for j in range(200) for x in (n0, sizes[j % len(sizes)])]
    salts = [x for j in range(200) for x in (salt0, 0x9_0000_0000 + j)]
    out = probe.reduce_probe(nv, 0, n, salts, values=1, blocking=blocking)
    assert np.isfinite(out).all()
    assert len({out[j, :nv].tobytes() for j in range(0, 400, 2)}) == 1
    assert len({out[j, :nv].tobytes() for j in range(1, 400, 2)}) > 100        # the neighbours did change
    assert [int(x) for x in out[:, nv]] == n


# ------------------------------------------------------------------ the LSM chains' hand-over
@pytest.mark.parametrize("nv", ref.HAND_OVER_NV)
def test_the_lsm_chains_hand_over_sums_exactly_in_every_workgroup(nv):
    """Form 3, what lsm_step_kernel and heston_lsm_step_kernel do between two dates: G1 workgroups store block_row_sum<nv> as plain rows,
    every one of G2 workgroups of the next launch sums all the rows by workgroup_rows_sum<nv>.  G1 = 1, 2, 255, 256, 257, 1024 (the
    chains' cap), each full, with one live thread in the last workgroup and with one thread missing; G2 = 1, 3, 256: EVERY workgroup's
    totals equal the integers."""
    n, salts = ref.hand_over_launches(nv)
    for g2 in ref.HAND_OVER_G2:
        for x, salt in zip(n, salts):
            out = probe.hand_over_probe(nv, x, salt, g2)
            want = expected(nv, x, salt)
            assert out.shape == (g2, nv) and np.isfinite(out).all(), (nv, g2, x)
            assert np.array_equal(out, np.floor(out)), (nv, g2, x, "a total that is not an integer")
            wrong = [(w, c, int(out[w, c]) - want[c]) for w in range(g2) for c in range(nv) if int(out[w, c]) != want[c]]
            assert not wrong, (nv, g2, f"n_threads {x} ({ref.workgroups(x)} workgroups), salt {salt:#x}", wrong[:4])


@pytest.mark.parametrize("nv", ref.HAND_OVER_NV)
def test_the_hand_over_s_rounded_totals_are_one_set_of_bits(nv):
    """values = 1 (sums round): all G2 workgroups hold the same bits, whatever G2 -- the rows are summed in index order by every
    workgroup -- and they lie within the bound of recursive summation of the correctly rounded sum (as the test above)."""
    n, salt = 256 * 257 - 3, 0xB_0000_0000 + nv
    fs, sabs, count = ref.rounded_reference(nv, n, salt)
    seen = set()
    for g2 in ref.HAND_OVER_G2:
        out = probe.hand_over_probe(nv, n, salt, g2, values=1)
        assert out.shape == (g2, nv) and np.isfinite(out).all()
        seen |= {out[w].tobytes() for w in range(g2)}
        for c in range(nv):
            assert abs(out[0, c] - fs[c]) <= count * 2.0 ** -53 * sabs[c], (nv, g2, c, out[0, c], fs[c])
    assert len(seen) == 1, (nv, len(seen))
    assert any(out[0, c] != math.floor(out[0, c]) for c in range(nv))            # the sums did round


# ------------------------------------------------------------------ tail and guard
@pytest.mark.parametrize("nv,form", ref.NV_FORMS)
def test_row_capacity_guard_answers_nan_through_the_tap_and_exact_sums_afterwards(nv, form):
    """The device-side bound check of grid_reduce / grid_reduce_workgroup through the tap (test_gpu_instrumented has it through
    prices): with the workspace REPORTING one value per row every launch refuses to store -- NaN totals, no tail, one group or
    several, blocking or queued -- and the next call without the knob is exact again (no counter left dirty)."""
    n, salts = [256 * 3 - 1, 256 * 300], [0xA_0000_0001, 0xA_0000_0002]
    probe.tune(probe.TUNE_FORCE_NV, 1)
    try:
        for blocking in (True, False):
            bad = probe.reduce_probe(nv, form, n, salts, values=0, blocking=blocking)
            assert np.isnan(bad[:, :nv]).all(), (blocking, bad)
            assert all(math.isnan(x) or x == -1.0 for x in bad[:, nv]), (blocking, bad[:, nv])
    finally:
        probe.tune(probe.TUNE_FORCE_NV, 0)
    for blocking in (True, False):
        assert_exact(probe.reduce_probe(nv, form, n, salts, values=0, blocking=blocking), nv, n, salts, (nv, form, "after the guard"))
