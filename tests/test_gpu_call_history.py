"""Every entry point gives the bits of a freshly initialised library whatever ran before it.

A context keeps state between calls: the reduction workspace (rows that are reallocated when a launch outgrows them, ticket counters
that reset themselves, the sequence number of the polled completion word), the bulk buffer, the batch workspace, the device copy of
the Sobol table with its host image, the bridge plan keyed by n, the Heston bridge slabs that only grow, the profiling event pools; and
the process keeps the tuning knobs and the profiling switch.  Every one of these is a cache whose key can be too coarse or a buffer
whose old contents or old capacity can show through.  The other GPU tests price in one fixed order each; here the calls of
tests/call_catalogue.py (one or more per compute entry point of include/olmc.h) run in many orders and every result is compared with the
BASELINE: the same call as the first one after olmc_shutdown + olmc_init, knobs at their defaults, profiling off.

The bar is bitwise everywhere: np.array_equal on the uint64 words of the results (call_catalogue.words).  A failure names the call, the
calls that ran before it and the first differing word with both values; after a whole-catalogue run the first failure is replayed once as
shutdown -> predecessor -> call, to say whether the immediate predecessor alone reproduces it.

No call here provokes a device error: the early returns of history 4 are argument errors (OLMC_ERR_ARG, refused before any device work)
and NaN inputs.  A bridge plan that fails its own checks cannot be requested through the ABI: qmc_bridge_plan's two failure returns
(overflow, incomplete) are unreachable for the n in [1, 1024] that the argument checks let through, so history 4 has no such call.
Should any call fail with something else than the refusal a history expects, every later test of this file fails at once without
touching the device again.
"""
import contextlib
import random

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import call_catalogue as cc
from tests.history import Device, baseline_fixture, first_difference

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

ENTRIES = cc.catalogue()
BY_NAME = {e.name: e for e in ENTRIES}
DEFAULT_KNOBS = ((_hip.TUNE_GRID_CAP, 0), (_hip.TUNE_QMC_BLOCK, 0), (_hip.TUNE_SPLIT_TAIL, 0), (_hip.TUNE_POLL, 0), (_hip.TUNE_SPLIT_SAT, 0),
                 (_hip.TUNE_MULTI_LAUNCH, 0), (_hip.TUNE_STAGED_COPY, 0), (_hip.TUNE_PHILOX_TABLE, 1))
DEVICE = Device()


def set_defaults():
    for knob, value in DEFAULT_KNOBS:
        _hip.tune(knob, value)
    _hip.profile_enable(False)


def run_history(sequence, expected, label):
    """Runs the entries one after the other on the library as it stands; every result against expected[name].  Returns the failures as
    (position in the sequence, report)."""
    failures, ran = [], []
    for pos, e in enumerate(sequence):
        got = DEVICE.invoke(e.name, e.call)
        if not np.array_equal(got, expected[e.name]):
            failures.append((pos, f"[{label}] {e.name} (call {pos + 1} of {len(sequence)}) differs from the fresh library: "
                                  f"{first_difference(got, expected[e.name])}\n    ran before it: {', '.join(ran) if ran else 'nothing'}"))
        ran.append(e.name)
    return failures


def report(failures, checks):
    if failures:
        pytest.fail(f"{len(failures)} of {checks} checks failed\n" + "\n".join(text for _, text in failures[:12]), pytrace=False)


# name -> words of the call on a fresh library; taken once.  Knobs at their defaults before, and again after the module.
baseline = baseline_fixture(DEVICE, lambda: {e.name: e.call for e in ENTRIES}, defaults=set_defaults)


def test_the_baseline_is_stable(baseline):
    """Five entries (one per kind of state) once more on a fresh library each: the yardstick itself has one value."""
    names = ["european-anti-N70001-n13", "multi-k70-N257-n5", "qmc-heston-bridge-n252-seedA-N100", "qmc-american-bridge-n13-seedA-N4133",
             "fetch-dev-N100-n64"]
    failures = []
    for name in names:
        got = DEVICE.fresh(name, BY_NAME[name].call)
        if not np.array_equal(got, baseline[name]):
            failures.append((0, f"{name} differs between two fresh libraries: {first_difference(got, baseline[name])}"))
    report(failures, len(names))


# ------------------------------------------------------------------------------------ 1. the whole catalogue, one library ----
def orders():
    yield "forward", list(ENTRIES)
    yield "reversed", list(reversed(ENTRIES))
    for k in range(3):
        seq = list(ENTRIES)
        random.Random(k).shuffle(seq)
        yield f"shuffle{k}", seq


@pytest.mark.parametrize("order", ["forward", "reversed", "shuffle0", "shuffle1", "shuffle2"])
def test_whole_catalogue_on_one_library(baseline, order):
    seq = dict(orders())[order]
    _hip.shutdown()
    failures = run_history(seq, baseline, order)
    if failures and failures[0][0] > 0:                       # ONE replay: does the immediate predecessor alone reproduce the first failure?
        pos, text = failures[0]
        before, e = seq[pos - 1], seq[pos]
        DEVICE.fresh(before.name, before.call)
        again = DEVICE.invoke(e.name, e.call)
        alone = not np.array_equal(again, baseline[e.name])
        failures[0] = (pos, text + f"\n    replay shutdown -> {before.name} -> {e.name}: the predecessor alone "
                                   + ("REPRODUCES it: " + first_difference(again, baseline[e.name]) if alone else "does NOT reproduce it"))
    report(failures, len(seq))


# ------------------------------------------------------------------------------------ 2. shrink after grow, per state tag ----
SIZE_KEYS = {
    "ws": lambda z: (z["N"] * max(z["k"], 1), z["n"]), "ws_wide": lambda z: (z["N"] * max(z["k"], 1), z["n"]),
    "caller_stream": lambda z: (z["N"], z["n"]), "bulk": lambda z: (z["N"] * (z["n"] + 1), z["n"]), "lsm": lambda z: (z["N"] * (z["n"] + 1), z["n"]),
    "multi": lambda z: (z["k"], z["N"]), "sobol": lambda z: (z["d"], z["N"]), "bridge": lambda z: (z["n"], z["N"]), "slabs": lambda z: (z["n"], z["N"]),
}


def by_size(tag):
    """The tag's entries from the largest shape to the smallest (the size that the tag's state is keyed or sized by)."""
    return sorted((e for e in ENTRIES if tag in e.state), key=lambda e: SIZE_KEYS[tag](e.sizes), reverse=True)


@pytest.mark.parametrize("tag", cc.STATE_TAGS)
def test_shrink_after_grow(baseline, tag):
    """Largest, smallest, one in between, largest again (n 252 -> 5 -> 64 -> 252, d 504 -> 5 -> 64 -> 504, N 70,001 -> 100 -> 4,133, k 70
    -> 3 -> 70); then every entry of the tag downwards and upwards again: the orders in which a buffer keeps its old capacity and a cache
    its old key."""
    down = by_size(tag)
    seq = [down[0], down[-1], down[len(down) // 2], down[0]] + down + down[::-1]
    _hip.shutdown()
    report(run_history(seq, baseline, f"shrink after grow: {tag}"), len(seq))


# ---------------------------------------------------------------------------------------- 3. same key, other contents ----
PAIRS = {
    "same d, other seed": [("qmc-european-d64-seedA-N4133", "qmc-european-d64-seedB-N4133"), ("qmc-batch-k3-d13-seedA-N4133", "qmc-cv-d13-seedB-N257"),
                           ("qmc-asian-bridge-n13-seedA-N257", "qmc-gbm-paths-sequential-time-major-n13-seedB-N100")],
    "same seed, other d": [("qmc-european-d64-seedA-N4133", "qmc-european-d128-seedA-N70001"), ("qmc-european-d5-seedA-N100", "qmc-european-d26-seedA-N257"),
                           ("qmc-barrier-bridge-n64-seedB-N257", "qmc-cv-d13-seedB-N257")],
    "a European d = a Heston 2n": [("qmc-european-d26-seedA-N257", "qmc-heston-bridge-n13-seedA-N257"),
                                   ("qmc-european-d128-seedA-N70001", "qmc-heston-sequential-n64-seedA-N4133"),
                                   ("qmc-terminal-plain-d128-seedA-N4133", "qmc-heston-paths-bridge-n64-seedA-N257")],
    "flat-vol bridge, Heston bridge, one n": [("qmc-asian-bridge-n13-seedA-N257", "qmc-heston-bridge-n13-seedA-N257"),
                                              ("qmc-asian-bridge-n252-seedA-N100", "qmc-heston-bridge-n252-seedA-N100"),
                                              ("qmc-barrier-bridge-n64-seedB-N257", "qmc-heston-path-payoff-bridge-n64-seedB-N257"),
                                              ("qmc-extrema-greeks-bridge-first-n64-seedA-N100", "qmc-heston-paths-bridge-n64-seedA-N257"),
                                              ("qmc-american-bridge-n13-seedA-N4133", "qmc-heston-surface-bridge-n13-seedA-N4133")],
    "Euler and QE on Sobol points, one n": [("qmc-heston-autocallable-euler-bridge-n64-seedA-N100", "qmc-heston-autocallable-qe-n64-seedA-N100"),
                                            ("qmc-heston-sequential-n64-seedA-N4133", "qmc-heston-qe-surface-n64-seedA-N257"),
                                            ("qmc-heston-paths-sequential-n13-seedA-N100", "qmc-heston-qe-paths-n13-seedA-N100"),
                                            ("qmc-heston-scenarios-bridge-n5-seedA-N257", "qmc-heston-cliquet-qe-n5-seedA-N100")],
}


@pytest.mark.parametrize("kind", list(PAIRS))
def test_same_key_other_contents(baseline, kind):
    """Each pair back to back, in both orders, from a fresh library and on a used one."""
    failures, checks = [], 0
    for a, b in PAIRS[kind]:
        for first, second in ((a, b), (b, a)):
            seq = [BY_NAME[first], BY_NAME[second], BY_NAME[first], BY_NAME[second]]
            _hip.shutdown()
            failures += run_history(seq, baseline, f"{kind}: {first} <-> {second}")
            checks += len(seq)
    report(failures, checks)


def test_american_chains_on_a_bulk_buffer_the_largest_matrix_filled(baseline):
    """The largest path matrices of the catalogue (Philox 65,537 x 65 doubles, Sobol 4,133 x 65) fill the bulk buffer; then the American
    Philox chain, the American Sobol chain and the boundaries read their own, smaller matrix, cash flows and rows out of it."""
    big = ["gbm-paths-time-major-N65537-n64", "qmc-gbm-paths-bridge-path-major-n64-seedA-N4133"]
    chain = ["american-put-N4133-n13", "qmc-american-bridge-n13-seedA-N4133", "boundary-put-N4133-n64"]
    rest = ["american-call-N257-n5", "qmc-american-sequential-n5-seedA-N257", "boundary-call-N100-n5", "qmc-boundary-bridge-n64-seedA-N257"]
    names = []
    for b in big:
        names += [b] + chain                                  # the issue's order on each of the two matrices
        for c in chain + rest:
            names += [b, c]                                   # and each of them directly behind the matrix
    names += chain[::-1] + rest[::-1]
    seq = [BY_NAME[n] for n in names]
    _hip.shutdown()
    report(run_history(seq, baseline, "American chains behind the largest matrix"), len(seq))


# -------------------------------------------------------------------------------------- 4. after a call that returned early ----
def _refused(call):
    """The call must be refused with OLMC_ERR_ARG."""
    def run(label):
        assert isinstance(DEVICE.guarded(label, call), ol.AccelerationError), f"{label}: was not refused"
    return run


def _nan(call):
    """A NaN input: the call succeeds and every price is NaN."""
    def run(label):
        got = DEVICE.guarded(label, call)
        got = got if isinstance(got, list) else [got]
        assert all(isinstance(st, _hip.Stats) and np.isnan(st.price) for st in got), (label, got)
    return run


H = cc.HESTON
EARLY = {
    "refused: n_steps = 0": _refused(lambda: _hip.european(*cc.EURO, True, 100, 0, cc.SEED, True)),
    "refused: bridge beyond 1024 dates": _refused(lambda: _hip.asian_qmc(*cc.QEURO, True, False, 100, *cc.tables(1025, cc.SEED_A), True, False)),
    "refused: Heston bridge beyond 1024 dates": _refused(
        lambda: _hip.heston_qmc(cc.QS, cc.QK, cc.QT, cc.QR, cc.HQ, True, *H, 100, *cc.tables(2050, cc.SEED_A), True, False)),
    "refused: QE with the bridge": _refused(
        lambda: _hip.heston_qe_qmc_surface(cc.QS, cc.QT, cc.QR, cc.HQ, True, *H, [100.0], [13], 100, *cc.tables(26, cc.SEED_B), True, False)),
    "refused: rho = 2": _refused(lambda: _hip.heston(cc.S, cc.K, cc.T, cc.R, cc.Q, True, H[0], H[1], H[2], 2.0, H[4], 257, 13, cc.SEED, False)),
    "refused: rho = 2 on the bridge": _refused(
        lambda: _hip.heston_qmc(cc.QS, cc.QK, cc.QT, cc.QR, cc.HQ, True, H[0], H[1], H[2], 2.0, H[4], 100, *cc.tables(26, cc.SEED_B), True, False)),
    "NaN spot": _nan(lambda: _hip.european(float("nan"), *cc.EURO[1:], True, 257, 5, cc.SEED, True)),
    "NaN contract in a batch": _nan(lambda: _hip.european_batch([(float("nan"), 100.0, 1.0, 0.05, 0.2, 0.0, True)] * 2, 257, 5, 42)),
    "NaN spot on Sobol bridge paths": _nan(lambda: _hip.asian_qmc(float("nan"), *cc.QEURO[1:], True, False, 100, *cc.tables(13, cc.SEED_B), True, False)),
    "NaN Heston scenarios": _nan(lambda: _hip.heston_qmc_scenarios([(float("nan"), 100.0, 1.0, 0.05, 0.02, True) + H] * 2, 100,
                                                                           *cc.tables(10, cc.SEED_B), True, False)),
}


@pytest.mark.parametrize("tag", cc.STATE_TAGS)
def test_after_a_call_that_returned_early(baseline, tag):
    """Every early return directly in front of every entry of the tag: a refused call must leave no half-made table, plan or workspace
    behind, and a NaN call (whose tables are another scramble's) none that the next call mistakes for its own."""
    entries = [e for e in ENTRIES if tag in e.state]
    _hip.shutdown()
    failures, checks = [], 0
    for label, early in EARLY.items():
        for e in entries:
            early(label)
            failures += run_history([e], baseline, f"{tag}, directly after '{label}'")
            checks += 1
    report(failures, checks)


# ------------------------------------------------------------------------------------------- 5. across the global switches ----
def picks():
    """Three entries per state tag -- the largest, the middle and the smallest shape -- without repeats."""
    seen, out = set(), []
    for tag in cc.STATE_TAGS:
        down = by_size(tag)
        for e in (down[0], down[len(down) // 2], down[-1]):
            if e.name not in seen:
                seen.add(e.name)
                out.append(e)
    return out


@contextlib.contextmanager
def knob(which, value, restore):
    _hip.tune(which, value)
    try:
        yield
    finally:
        _hip.tune(which, restore)


@contextlib.contextmanager
def profiling():
    _hip.profile_enable(True)
    try:
        yield
    finally:
        _hip.profile_enable(False)


SAME_BITS = {
    "poll": [lambda: knob(_hip.TUNE_POLL, -1, 0)],
    "philox table": [lambda: knob(_hip.TUNE_PHILOX_TABLE, 0, 1)],
    "staged copy": [lambda: knob(_hip.TUNE_STAGED_COPY, -1, 0)],
}


@pytest.mark.parametrize("switch", list(SAME_BITS))
def test_switches_that_promise_the_same_bits(baseline, switch):
    """olmc.h: same bits under the Philox table, the wait by polling and the staged copy.  The baseline's bits while the switch is set,
    and again once it is back."""
    seq = picks()
    _hip.shutdown()
    failures, checks = [], 0
    for i, setting in enumerate(SAME_BITS[switch]):
        with setting():
            failures += run_history(seq, baseline, f"{switch}, setting {i + 1}")
        failures += run_history(seq, baseline, f"{switch}, back at the default after setting {i + 1}")
        checks += 2 * len(seq)
    report(failures, checks)


@pytest.mark.parametrize("shape", [-1, 1, 2])
def test_sobol_block_shapes(baseline, shape):
    """OLMC_TUNE_QMC_BLOCK.  olmc.h promises the same TERMINAL PRICES bit for bit under every shape (one association of a point's normal
    sum): the terminal arrays keep the baseline's bits while the knob is set, and so does every call that is not a European Sobol
    launch.  The payoff SUMS over the points are the same points in another association -- a thread that carries eight points adds its
    eight payoffs before the workgroup's tree does (measured here: qmc-european-d5-seedA-N100 under shape 1, sumsq 0x40e003323761a5a2
    against 0x40e003323761a5a1) -- so they are held to the same call under the same shape on a fresh library.  Back at the default
    everything has the baseline's bits again."""
    seq = picks() + [e for e in ENTRIES if e.entry_points == ("olmc_european_qmc_terminal",) and e not in picks()]
    shaped = {"olmc_european_qmc", "olmc_european_qmc_cv", "olmc_european_qmc_batch", "olmc_european_qmc_greeks_fd", "olmc_multi_gpu_european_qmc",
              "olmc_multi_gpu_european_qmc_greeks_fd", "olmc_multi_gpu_european_qmc_cv"}
    failures = []
    with knob(_hip.TUNE_QMC_BLOCK, shape, 0):
        expected = {e.name: DEVICE.fresh(e.name, e.call) if shaped & set(e.entry_points) else baseline[e.name] for e in seq}
        _hip.shutdown()
        failures += run_history(seq, expected, f"Sobol block shape {shape}")
        failures += run_history(seq[::-1], expected, f"Sobol block shape {shape}, reversed")
    failures += run_history(seq, baseline, f"back at the default after Sobol block shape {shape}")
    report(failures, 3 * len(seq))


def test_profiling_on_and_off(baseline):
    """Profiling attaches events to the launches and keeps its pools with the context: same bits while it is on, with the time read and
    reset in between, and after it is off again."""
    seq = picks()
    _hip.shutdown()
    failures = []
    with profiling():
        failures += run_history(seq, baseline, "profiling on")
        launches, ms = _hip.kernel_time()
        assert launches >= 1 and ms > 0.0, (launches, ms)
        _hip.profile_reset()
        assert _hip.kernel_time()[0] == 0
        failures += run_history(seq[::-1], baseline, "profiling on, after the reset")
    failures += run_history(seq, baseline, "profiling off again")
    report(failures, 3 * len(seq))


OTHER_ASSOCIATION = {"grid cap": (_hip.TUNE_GRID_CAP, 1, 0), "split tail": (_hip.TUNE_SPLIT_TAIL, -1, 0)}


@pytest.mark.parametrize("switch", list(OTHER_ASSOCIATION))
def test_switches_that_change_the_association(baseline, switch):
    """olmc.h: the grid cap and the split tail keep the paths and change the launch shape, so sums may associate otherwise.  Under the
    switch the bits are those of the SAME switched call on a fresh library; back at the default they are the baseline's."""
    which, value, default = OTHER_ASSOCIATION[switch]
    seq = picks()
    failures = []
    with knob(which, value, default):
        switched = {e.name: DEVICE.fresh(e.name, e.call) for e in seq}
        _hip.shutdown()
        failures += run_history(seq, switched, f"{switch} set")
        failures += run_history(seq[::-1], switched, f"{switch} set, reversed")
    failures += run_history(seq, baseline, f"{switch} back at the default")
    with knob(which, value, default):
        failures += run_history(seq, switched, f"{switch} set again on the used library")
    failures += run_history(seq[::-1], baseline, f"{switch} back at the default again")
    report(failures, 5 * len(seq))
