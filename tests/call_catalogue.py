"""One small deterministic call per compute entry point of include/olmc.h, for tests/test_gpu_call_history.py.

A helper, not a test module.  Every entry is (name, the olmc_* symbols it reaches, a zero-argument callable through optionslab_amd._hip,
the state of the library's context it touches, its sizes).  An entry point has several entries where its forms use different state
(antithetic, bridge / sequential, path_major, Euler / QE, first / second order, prices only).  Nothing here is an oracle: the history
test compares a call with THE SAME call on a freshly initialised library, bit for bit.  The contracts are those the oracle tests
already price -- tests/test_gpu_grid_stride.py's (S, K, T, R, SIG, Q), SEED, MERTON, KOU, AUTOCALL, CLIQUET, its N = 257 x 5 steps;
tests/test_gpu_exotic_qmc.py's at-the-money contract with UP / DOWN and the seeds 7 and 1234; tests/heston_path_oracle.py's and
tests/heston_qe_reference.py's USUAL model; tests/test_gpu_american_qmc.py's CASES -- at the smallest shapes at which the kept state
still differs between entries:
    paths / points  100, 257, 4133; one 70,001-path European (more than 256 workgroups: a second reduction group); european_multi of
                    70 and of 3 contracts (the batch workspace's two sizes);
                    one path matrix of 65,537 x 65 doubles (34 MB: the only result large enough for the staged copy and its pinned buffers);
    steps           5, 13, 64; one 252-step bridge call each for the flat-vol and the Heston Sobol kernels (plan and slab growth);
    Sobol tables    d in {5, 13, 26, 64, 128, 252, 504}; d = 64 and d = 13 come with two seeds; seed 7 comes with every d; the Heston
                    calls of 13 steps read the d = 26 table of seed 7 that a European call reads too (the same table for two families).
The tables come from optionslab_amd.monte_carlo.sobol_tables, as in the oracle tests.

State tags: "ws" the reduction workspace of the library's own stream (rows, group rows, ticket counters, the polled completion word);
"ws_wide" the same with rows of more than two values or more than one reduction group; "bulk" the bulk buffer (terminal arrays, path
matrices, the validation taps); "multi" olmc_european_multi's batch workspace; "sobol" the device copy of the Sobol table; "bridge" the
bridge plan; "slabs" the Heston bridge slabs; "lsm" the American chain (matrix, cash flows and regression rows in the bulk buffer);
"caller_stream" a reduction workspace claimed by a caller's stream.  The single-process multi-GPU entry points run with n_gpus = 1: their
rank owns a context of its own (workspace and table), torn down by olmc_shutdown like context 0.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Callable, Dict, FrozenSet, List, NamedTuple, Tuple

import numpy as np

from optionslab_amd import _hip

STATE_TAGS = ("ws", "ws_wide", "bulk", "multi", "sobol", "bridge", "slabs", "lsm", "caller_stream")


class Entry(NamedTuple):
    name: str
    entry_points: Tuple[str, ...]      # the olmc_* symbols the call reaches
    call: Callable[[], object]
    state: FrozenSet[str]
    sizes: Dict[str, int]              # N paths / points, n steps, d Sobol dimensions, k contracts (0: not applicable)


# ------------------------------------------------------------------------------------------------ results as words ----
def _bytes_of(x) -> bytes:
    if isinstance(x, _hip.Stats):
        return struct.pack("<ddqdd", x.sum, x.sumsq, x.n, x.price, x.std_error)
    if isinstance(x, _hip.CvMoments):
        return struct.pack("<dddddqd", x.sum_d, x.sum_s, x.sum_dd, x.sum_ss, x.sum_ds, x.n, x.value)
    if isinstance(x, np.ndarray):
        b = np.ascontiguousarray(x).tobytes()
        return b + b"\0" * (-len(b) % 8)
    if isinstance(x, (list, tuple)):
        return b"".join(_bytes_of(y) for y in x)
    if isinstance(x, float):
        return struct.pack("<d", x)
    if isinstance(x, (int, np.integer)):
        return struct.pack("<q", int(x))
    raise TypeError(f"no byte image for a {type(x).__name__}")


def words(result) -> np.ndarray:
    """The result as uint64 words: a Stats is (sum, sumsq, n, price, std_error), a CvMoments its seven fields, arrays and lists of
    floats their doubles, tuples and lists one after the other.  -0.0, NaN payloads and last bits all count."""
    return np.frombuffer(_bytes_of(result), dtype=np.uint64).copy()


# ------------------------------------------------------------------------------------------------------ arguments ----
S, K, T, R, SIG, Q = 100.0, 105.0, 1.0, 0.05, 0.2, 0.01           # tests/test_gpu_grid_stride.py
SEED = (0x9E3779B9 << 32) | 20240229
MERTON, KOU = (False, 1.0, -0.1, 0.2, 0.0), (True, 1.0, 0.4, 10.0, 5.0)
AUTOCALL = (1.0, 0.9, 0.1, 0.8)
CLIQUET = (0.05, -0.05, 0.5, 0.0)
HESTON = (2.0, 0.04, 0.3, -0.7, 0.04)                               # USUAL of tests/heston_path_oracle.py and tests/heston_qe_reference.py
QS, QK, QT, QR, QSIG, QQ = 100.0, 100.0, 1.0, 0.05, 0.2, 0.0        # tests/test_gpu_exotic_qmc.py
UP, DOWN = 115.0, 88.0
HQ = 0.01                                                           # tests/test_gpu_heston_qmc.py's dividend yield
SEED_A, SEED_B = 7, 1234
STRIKES = (80.0, 100.0, 120.0)                                      # tests/test_gpu_heston_surface.py
BARRIER_UP_OUT, BARRIER_DOWN_IN = 0, 3
OBS = {5: 2, 13: 4, 64: 21, 252: 21}                                # observation frequency / periods by steps (test_gpu_heston_structured.py SHAPES)
PER = {5: 5, 13: 4, 64: 12, 252: 12}
EURO = (S, K, T, R, SIG, Q)
QEURO = (QS, QK, QT, QR, QSIG, QQ)
BATCH3 = [(100.0, 100.0, 1.0, 0.05, 0.2, 0.0, True), (101.0, 100.0, 1.0, 0.05, 0.2, 0.0, True),
          (99.0, 95.0, 0.5, 0.03, 0.25, 0.01, False)]              # tests/test_gpu_parity.py test_batch_equals_separate_launches
TABLE_POINTS = 1 << 17                                              # every table knows the columns of the largest call (70,001 points)

_tables: dict = {}


def tables(d: int, seed: int):
    """(sv, shift) of the d-dimensional scramble `seed`, built once (the package's own helper keeps only eight tables)."""
    key = (d, seed)
    if key not in _tables:
        from optionslab_amd.monte_carlo import sobol_tables
        _tables[key] = sobol_tables(d, seed, TABLE_POINTS)
    return _tables[key]


_torch_state: dict = {}


def caller_stream():
    """(torch, a stream, a buffer of 3 doubles on the device), as test_fetch_dev_hands_over_what_earlier_work_on_the_stream_left."""
    if not _torch_state:
        import torch
        _hip.lib()
        _torch_state["torch"] = torch
        _torch_state["stream"] = torch.cuda.Stream()
        _torch_state["buf"] = torch.zeros(3, dtype=torch.float64, device="cuda")
    return _torch_state["torch"], _torch_state["stream"], _torch_state["buf"]


def _shard_dev(N, n, seed, own_stream: bool):
    torch, st, buf = caller_stream()
    buf.zero_()
    torch.cuda.synchronize()
    ptr = st.cuda_stream if own_stream else 0
    with torch.cuda.stream(st):
        _hip.european_shard_dev(*EURO, True, 1000, N, n, seed, True, buf.data_ptr(), ptr)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _fetch_dev(N, n, seed):
    torch, st, buf = caller_stream()
    buf.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        _hip.european_shard_dev(*EURO, True, 1000, N, n, seed, True, buf.data_ptr(), st.cuda_stream)
        got = _hip.fetch_dev(buf.data_ptr(), 3, st.cuda_stream)
    torch.cuda.synchronize()
    return np.array(got, dtype=np.float64)


def _european_direct(N, n, anti):
    out = _hip.Stats()
    _hip._check(_hip.lib().olmc_european(*EURO, 1, N, n, _hip.seed64(SEED), int(anti), C.byref(out)))
    return out


def _multi(k, N, n):
    i = np.arange(k, dtype=np.float64)
    return _hip.european_multi(95.0 + (i % 11), 100.0 + (i % 7), 0.5 + 0.125 * (i % 5), 0.05, 0.15 + 0.01 * (i % 9), 0.01, (i % 2 == 0), N, n, SEED, True)


def _scenario_set():
    """Four scenarios on three recursions (the model of one differs, the maturity of another)."""
    other = (1.5, 0.09, 0.1, -0.5, 0.1)                             # CALM_OTHER of tests/test_gpu_heston_scenarios.py
    return [(100.0, 100.0, 1.0, 0.05, 0.02, True) + HESTON, (105.0, 95.0, 1.0, 0.03, 0.0, False) + HESTON,
            (100.0, 110.0, 0.5, 0.05, 0.02, True) + HESTON, (100.0, 100.0, 1.0, 0.05, 0.02, True) + other]


def _cells(n):
    return list(STRIKES), [n, max(n // 2, 1), max(n // 4, 1)]


# ------------------------------------------------------------------------------------------------------ catalogue ----
def catalogue() -> List[Entry]:
    h = _hip
    out: List[Entry] = []

    def add(name, entry_points, state, call, N=0, n=0, d=0, k=0):
        eps = (entry_points,) if isinstance(entry_points, str) else tuple(entry_points)
        tags = frozenset(state.split())
        assert tags <= set(STATE_TAGS), (name, tags)
        out.append(Entry(name, eps, call, tags, dict(N=N, n=n, d=d, k=k)))

    # ---- Philox: European family
    add("european-direct-anti-N257-n5", "olmc_european", "ws", lambda: _european_direct(257, 5, True), N=257, n=5)
    add("european-anti-N4133-n13", "olmc_european_shard", "ws", lambda: h.european(*EURO, True, 4133, 13, SEED, True, path_offset=2**32 - 100), N=4133, n=13)
    add("european-plain-N100-n64", "olmc_european_shard", "ws", lambda: h.european(*EURO, False, 100, 64, SEED, False), N=100, n=64)
    add("european-anti-N70001-n13", "olmc_european_shard", "ws ws_wide", lambda: h.european(*EURO, True, 70_001, 13, SEED, True), N=70_001, n=13)
    add("european-anti-N257-n252", "olmc_european_shard", "ws", lambda: h.european(*EURO, True, 257, 252, SEED, True), N=257, n=252)
    add("shard-dev-own-stream-N4133-n13", "olmc_european_shard_dev", "caller_stream", lambda: _shard_dev(4133, 13, 5, True), N=4133, n=13)
    add("shard-dev-null-stream-N257-n5", "olmc_european_shard_dev", "caller_stream", lambda: _shard_dev(257, 5, 6, False), N=257, n=5)
    add("fetch-dev-N100-n64", ("olmc_european_shard_dev", "olmc_fetch_dev"), "caller_stream ws", lambda: _fetch_dev(100, 64, 7), N=100, n=64)
    add("batch-k3-N257-n5", "olmc_european_batch", "ws ws_wide", lambda: h.european_batch(BATCH3, 257, 5, 42), N=257, n=5, k=3)
    add("batch-k16-plain-N4133-n13", "olmc_european_batch", "ws ws_wide",
        lambda: h.european_batch([(100.0 + i, 100.0, 1.0, 0.05, 0.2, 0.0, True) for i in range(16)], 4133, 13, 1, antithetic=False), N=4133, n=13, k=16)
    add("multi-k70-N257-n5", "olmc_european_multi", "multi", lambda: _multi(70, 257, 5), N=257, n=5, k=70)
    add("multi-k3-N4133-n13", "olmc_european_multi", "multi", lambda: _multi(3, 4133, 13), N=4133, n=13, k=3)
    add("multi-k3-N70001-n5", "olmc_european_multi", "multi", lambda: _multi(3, 70_001, 5), N=70_001, n=5, k=3)
    add("greeks-first-N257-n5", "olmc_european_greeks_fd", "ws ws_wide", lambda: h.european_greeks_fd(*EURO, True, 257, 5, SEED, False), N=257, n=5, k=8)
    add("greeks-second-N4133-n13", "olmc_european_greeks_fd", "ws ws_wide", lambda: h.european_greeks_fd(*EURO, False, 4133, 13, SEED, True), N=4133, n=13, k=14)
    add("greeks-prices-only-N100-n64", "olmc_european_greeks_fd", "ws ws_wide",
        lambda: h.european_greeks_fd(*EURO, True, 100, 64, SEED, True, want_evals=False), N=100, n=64, k=14)
    add("terminal-anti-N257-n5", "olmc_european_terminal", "bulk", lambda: h.european_terminal(S, T, R, SIG, Q, 257, 5, SEED, True), N=514, n=1)
    add("terminal-plain-N4133-n13", "olmc_european_terminal", "bulk", lambda: h.european_terminal(S, T, R, SIG, Q, 4133, 13, SEED, False), N=4133, n=1)
    add("gbm-paths-time-major-N257-n13", "olmc_gbm_paths", "bulk", lambda: h.gbm_paths(S, T, R, SIG, Q, 257, 13, SEED, False), N=257, n=13)
    add("gbm-paths-path-major-N4133-n64", "olmc_gbm_paths", "bulk", lambda: h.gbm_paths(S, T, R, SIG, Q, 4133, 64, SEED, True), N=4133, n=64)
    add("gbm-paths-time-major-N65537-n64", "olmc_gbm_paths", "bulk", lambda: h.gbm_paths(S, T, R, SIG, Q, 65_537, 64, SEED, False), N=65_537, n=64)   # 34 MB: the staged copy
    add("cv-anti-N257-n5", "olmc_european_cv", "ws ws_wide", lambda: h.european_cv(*EURO, True, 257, 5, SEED, True), N=257, n=5, k=5)
    add("cv-shard-plain-N4133-n13", "olmc_european_cv_shard", "ws ws_wide", lambda: h.european_cv_shard(*EURO, False, 2**32 - 100, 4133, 13, SEED, False), N=4133, n=13, k=5)

    # ---- Philox: path payoffs, structured products, American, Heston, jumps
    add("asian-arithmetic-anti-N257-n5", "olmc_asian", "ws", lambda: h.asian(*EURO, True, False, 257, 5, SEED, True), N=257, n=5)
    add("asian-geometric-N4133-n64", "olmc_asian", "ws", lambda: h.asian(*EURO, False, True, 4133, 64, SEED, False), N=4133, n=64)
    add("asian-fast-N100-n13", "olmc_asian", "ws", lambda: h.asian(*EURO, True, False, 100, 13, SEED, False, fast=True), N=100, n=13)
    add("asian-greeks-arithmetic-second-N257-n13", "olmc_asian_greeks_fd", "ws ws_wide", lambda: h.asian_greeks_fd(*EURO, True, 257, 13, SEED, True, True), N=257, n=13, k=14)
    add("asian-greeks-geometric-first-N100-n5", "olmc_asian_greeks_fd", "ws ws_wide",
        lambda: h.asian_greeks_fd(*EURO, False, 100, 5, SEED, False, False, geometric=True), N=100, n=5, k=8)
    add("barrier-up-out-anti-N257-n5", "olmc_barrier", "ws", lambda: h.barrier(*EURO, True, UP, BARRIER_UP_OUT, 257, 5, SEED, True), N=257, n=5)
    add("barrier-down-in-N4133-n64", "olmc_barrier", "ws", lambda: h.barrier(*EURO, False, DOWN, BARRIER_DOWN_IN, 4133, 64, SEED, False), N=4133, n=64)
    add("lookback-floating-N257-n13", "olmc_lookback", "ws", lambda: h.lookback(*EURO, True, False, 257, 13, SEED, False), N=257, n=13)
    add("lookback-fixed-anti-N100-n5", "olmc_lookback", "ws", lambda: h.lookback(*EURO, False, True, 100, 5, SEED, True), N=100, n=5)
    add("extrema-greeks-barrier-first-N257-n5", "olmc_extrema_greeks_fd", "ws ws_wide",
        lambda: h.extrema_greeks_fd(*EURO, True, BARRIER_UP_OUT, UP, 257, 5, SEED, False, False), N=257, n=5, k=8)
    add("extrema-greeks-lookback-second-N100-n13", "olmc_extrema_greeks_fd", "ws ws_wide",
        lambda: h.extrema_greeks_fd(*EURO, False, h.LOOKBACK_FIXED, 0.0, 100, 13, SEED, True, True), N=100, n=13, k=14)
    add("autocallable-N257-n5", "olmc_autocallable", "ws", lambda: h.autocallable(S, T, R, SIG, Q, *AUTOCALL, OBS[5], 257, 5, SEED, True), N=257, n=5)
    add("cliquet-N4133-n13", "olmc_cliquet", "ws", lambda: h.cliquet(S, T, R, SIG, Q, *CLIQUET, PER[13], 4133, 13, SEED, False), N=4133, n=13)
    add("american-put-N4133-n13", "olmc_american_lsm", "lsm bulk ws", lambda: h.american_lsm(95.0, 100.0, 1.0, 0.05, 0.15, 0.0, False, 4133, 13, 3, 7), N=4133, n=13)
    add("american-call-N257-n5", "olmc_american_lsm", "lsm bulk ws", lambda: h.american_lsm(100.0, 90.0, 1.0, 0.05, 0.25, 0.05, True, 257, 5, 1, 7), N=257, n=5)
    add("boundary-put-N4133-n64", "olmc_exercise_boundary", "lsm bulk", lambda: h.exercise_boundary(100.0, 100.0, 1.0, 0.05, 0.2, 0.0, False, 4133, 64, 7), N=4133, n=64)
    add("boundary-call-N100-n5", "olmc_exercise_boundary", "lsm bulk", lambda: h.exercise_boundary(100.0, 100.0, 1.0, 0.05, 0.2, 0.05, True, 100, 5, 7), N=100, n=5)
    add("heston-anti-N257-n5", "olmc_heston", "ws", lambda: h.heston(S, K, T, R, Q, True, *HESTON, 257, 5, SEED, True), N=257, n=5)
    add("heston-paths-path-major-N257-n13", "olmc_heston_paths", "bulk", lambda: h.heston_paths(S, T, R, Q, *HESTON, 257, 13, SEED, True), N=514, n=13)
    add("heston-paths-time-major-N100-n64", "olmc_heston_paths", "bulk", lambda: h.heston_paths(S, T, R, Q, *HESTON, 100, 64, SEED, False), N=200, n=64)
    add("merton-N257-n5", "olmc_jump_diffusion", "ws", lambda: h.jump_diffusion(*EURO, True, *MERTON, 257, 5, SEED), N=257, n=5)
    add("kou-N4133-n13", "olmc_jump_diffusion", "ws", lambda: h.jump_diffusion(*EURO, False, *KOU, 4133, 13, SEED, path_offset=2**32 - 100), N=4133, n=13)
    add("jump-paths-kou-N257-n5", "olmc_jump_paths", "bulk", lambda: h.jump_paths(S, T, R, SIG, Q, *KOU, 257, 5, SEED, True), N=257, n=5)
    add("heston-path-payoff-asian-N257-n13", "olmc_heston_path_payoff", "ws",
        lambda: h.heston_path_payoff(S, K, T, R, Q, True, *HESTON, h.PATH_ASIAN_ARITHMETIC, 0.0, 257, 13, SEED, True), N=257, n=13)
    add("heston-surface-N4133-n13", "olmc_heston_surface", "ws ws_wide", lambda: h.heston_surface(S, T, R, Q, True, *HESTON, *_cells(13), 4133, 13, SEED, False), N=4133, n=13, k=3)
    add("heston-scenarios-N257-n5", "olmc_heston_scenarios", "ws ws_wide", lambda: h.heston_scenarios(_scenario_set(), 257, 5, SEED, True), N=257, n=5, k=4)
    add("heston-greeks-second-N257-n13", "olmc_heston_greeks_fd", "ws ws_wide",
        lambda: h.heston_greeks_fd(*EURO, True, *HESTON[:4], 257, 13, SEED, False, True), N=257, n=13, k=14)
    add("heston-qe-surface-N4133-n13", "olmc_heston_qe_surface", "ws ws_wide", lambda: h.heston_qe_surface(S, T, R, Q, False, *HESTON, *_cells(13), 4133, 13, 3, True), N=4133, n=13, k=3)
    add("heston-qe-paths-N257-n5", "olmc_heston_qe_paths", "bulk", lambda: h.heston_qe_paths(S, T, R, Q, *HESTON, 257, 5, 3, False), N=514, n=5)
    add("heston-autocallable-euler-N257-n13", "olmc_heston_autocallable", "ws", lambda: h.heston_autocallable(S, T, R, Q, *HESTON, *AUTOCALL, OBS[13], 257, 13, SEED, True), N=257, n=13)
    add("heston-autocallable-qe-N100-n5", "olmc_heston_autocallable", "ws", lambda: h.heston_autocallable(S, T, R, Q, *HESTON, *AUTOCALL, OBS[5], 100, 5, SEED, False, qe=True), N=100, n=5)
    add("heston-cliquet-euler-N100-n64", "olmc_heston_cliquet", "ws", lambda: h.heston_cliquet(S, T, R, Q, *HESTON, *CLIQUET, PER[64], 100, 64, SEED, False), N=100, n=64)
    add("heston-cliquet-qe-N257-n13", "olmc_heston_cliquet", "ws", lambda: h.heston_cliquet(S, T, R, Q, *HESTON, *CLIQUET, PER[13], 257, 13, SEED, True, qe=True), N=257, n=13)
    add("philox-words-N257", "olmc_philox_words", "bulk", lambda: h.philox_words(SEED, 2**32 - 100, 257, 1, 3, 2), N=257, n=3)
    add("normals-N100-n13", "olmc_normals", "bulk", lambda: h.normals(SEED, 0, 100, 13), N=100, n=7)

    # ---- Sobol: European family (d Sobol dimensions)
    add("qmc-european-d64-seedA-N4133", "olmc_european_qmc", "sobol ws", lambda: h.european_qmc(*QEURO, True, 4133, *tables(64, SEED_A)), N=4133, d=64)
    add("qmc-european-d64-seedB-N4133", "olmc_european_qmc", "sobol ws", lambda: h.european_qmc(*QEURO, True, 4133, *tables(64, SEED_B)), N=4133, d=64)
    add("qmc-european-d26-seedA-N257", "olmc_european_qmc", "sobol ws", lambda: h.european_qmc(*QEURO, False, 257, *tables(26, SEED_A), point_offset=64), N=257, d=26)
    add("qmc-european-d128-seedA-N70001", "olmc_european_qmc", "sobol ws ws_wide", lambda: h.european_qmc(*QEURO, True, 70_001, *tables(128, SEED_A)), N=70_001, d=128)
    add("qmc-european-d5-seedA-N100", "olmc_european_qmc", "sobol ws", lambda: h.european_qmc(*QEURO, True, 100, *tables(5, SEED_A)), N=100, d=5)
    add("qmc-cv-d13-seedB-N257", "olmc_european_qmc_cv", "sobol ws ws_wide", lambda: h.european_qmc_cv(*QEURO, True, 257, *tables(13, SEED_B)), N=257, d=13, k=5)
    add("qmc-batch-k3-d13-seedA-N4133", "olmc_european_qmc_batch", "sobol ws ws_wide", lambda: h.european_qmc_batch(BATCH3, 4133, *tables(13, SEED_A)), N=4133, d=13, k=3)
    add("qmc-greeks-first-d5-seedA-N257", "olmc_european_qmc_greeks_fd", "sobol ws ws_wide", lambda: h.european_qmc_greeks_fd(*QEURO, True, 257, *tables(5, SEED_A), False), N=257, d=5, k=8)
    add("qmc-greeks-second-d64-seedA-N100", "olmc_european_qmc_greeks_fd", "sobol ws ws_wide", lambda: h.european_qmc_greeks_fd(*QEURO, False, 100, *tables(64, SEED_A), True), N=100, d=64, k=14)
    add("qmc-terminal-anti-d13-seedA-N257", "olmc_european_qmc_terminal", "sobol bulk", lambda: h.european_qmc_terminal(QS, QT, QR, QSIG, QQ, 257, *tables(13, SEED_A), antithetic=True), N=514, n=1, d=13)
    add("qmc-terminal-plain-d128-seedA-N4133", "olmc_european_qmc_terminal", "sobol bulk", lambda: h.european_qmc_terminal(QS, QT, QR, QSIG, QQ, 4133, *tables(128, SEED_A)), N=4133, n=1, d=128)

    # ---- Sobol: flat-vol path kernels (n steps = d dimensions)
    add("qmc-asian-bridge-n13-seedA-N257", "olmc_asian_qmc", "sobol bridge ws", lambda: h.asian_qmc(*QEURO, True, False, 257, *tables(13, SEED_A), True, True), N=257, n=13, d=13)
    add("qmc-asian-sequential-n64-seedA-N4133", "olmc_asian_qmc", "sobol ws", lambda: h.asian_qmc(*QEURO, False, True, 4133, *tables(64, SEED_A), False, False), N=4133, n=64, d=64)
    add("qmc-asian-bridge-n252-seedA-N100", "olmc_asian_qmc", "sobol bridge ws", lambda: h.asian_qmc(*QEURO, True, False, 100, *tables(252, SEED_A), True, False), N=100, n=252, d=252)
    add("qmc-barrier-bridge-n64-seedB-N257", "olmc_extrema_qmc", "sobol bridge ws", lambda: h.extrema_qmc(*QEURO, True, BARRIER_UP_OUT, UP, 257, *tables(64, SEED_B), True, False), N=257, n=64, d=64)
    add("qmc-lookback-sequential-n5-seedA-N100", "olmc_extrema_qmc", "sobol ws", lambda: h.extrema_qmc(*QEURO, False, h.LOOKBACK_FLOATING, 0.0, 100, *tables(5, SEED_A), False, True), N=100, n=5, d=5)
    add("qmc-asian-greeks-bridge-second-n13-seedA-N257", "olmc_asian_qmc_greeks_fd", "sobol bridge ws ws_wide",
        lambda: h.asian_qmc_greeks_fd(*QEURO, True, False, 257, *tables(13, SEED_A), True, False, True), N=257, n=13, d=13, k=14)
    add("qmc-asian-greeks-sequential-first-n5-seedA-N100", "olmc_asian_qmc_greeks_fd", "sobol ws ws_wide",
        lambda: h.asian_qmc_greeks_fd(*QEURO, False, True, 100, *tables(5, SEED_A), False, True, False), N=100, n=5, d=5, k=8)
    add("qmc-extrema-greeks-bridge-first-n64-seedA-N100", "olmc_extrema_qmc_greeks_fd", "sobol bridge ws ws_wide",
        lambda: h.extrema_qmc_greeks_fd(*QEURO, True, BARRIER_DOWN_IN, DOWN, 100, *tables(64, SEED_A), True, False, False), N=100, n=64, d=64, k=8)
    add("qmc-extrema-greeks-sequential-second-n13-seedB-N257", "olmc_extrema_qmc_greeks_fd", "sobol ws ws_wide",
        lambda: h.extrema_qmc_greeks_fd(*QEURO, False, h.LOOKBACK_FIXED, 0.0, 257, *tables(13, SEED_B), False, True, True), N=257, n=13, d=13, k=14)
    add("qmc-autocallable-bridge-n13-seedA-N257", "olmc_autocallable_qmc", "sobol bridge ws", lambda: h.autocallable_qmc(QS, QT, QR, QSIG, QQ, *AUTOCALL, OBS[13], 257, *tables(13, SEED_A), True, True), N=257, n=13, d=13)
    add("qmc-cliquet-sequential-n64-seedA-N100", "olmc_cliquet_qmc", "sobol ws", lambda: h.cliquet_qmc(QS, QT, QR, QSIG, QQ, *CLIQUET, PER[64], 100, *tables(64, SEED_A), False, False), N=100, n=64, d=64)
    add("qmc-american-bridge-n13-seedA-N4133", "olmc_american_lsm_qmc", "sobol bridge lsm bulk ws",
        lambda: h.american_lsm_qmc(95.0, 100.0, 1.0, 0.05, 0.15, 0.0, False, 4133, *tables(13, SEED_A), True, 3), N=4133, n=13, d=13)
    add("qmc-american-sequential-n5-seedA-N257", "olmc_american_lsm_qmc", "sobol lsm bulk ws",
        lambda: h.american_lsm_qmc(100.0, 90.0, 1.0, 0.05, 0.25, 0.05, True, 257, *tables(5, SEED_A), False, 1), N=257, n=5, d=5)
    add("qmc-boundary-bridge-n64-seedA-N257", "olmc_exercise_boundary_qmc", "sobol bridge lsm bulk",
        lambda: h.exercise_boundary_qmc(100.0, 100.0, 1.0, 0.05, 0.2, 0.0, False, 257, *tables(64, SEED_A), True), N=257, n=64, d=64)
    add("qmc-gbm-paths-bridge-path-major-n64-seedA-N4133", "olmc_gbm_qmc_paths", "sobol bridge bulk",
        lambda: h.gbm_qmc_paths(QS, QT, QR, QSIG, QQ, 4133, *tables(64, SEED_A), True, True), N=4133, n=64, d=64)
    add("qmc-gbm-paths-sequential-time-major-n13-seedB-N100", "olmc_gbm_qmc_paths", "sobol bulk",
        lambda: h.gbm_qmc_paths(QS, QT, QR, QSIG, QQ, 100, *tables(13, SEED_B), False, False), N=100, n=13, d=13)

    # ---- Sobol: Heston (n steps = d / 2)
    add("qmc-heston-bridge-n13-seedA-N257", "olmc_heston_qmc", "sobol bridge slabs ws", lambda: h.heston_qmc(QS, QK, QT, QR, HQ, True, *HESTON, 257, *tables(26, SEED_A), True, True), N=257, n=13, d=26)
    add("qmc-heston-sequential-n64-seedA-N4133", "olmc_heston_qmc", "sobol ws", lambda: h.heston_qmc(QS, QK, QT, QR, HQ, False, *HESTON, 4133, *tables(128, SEED_A), False, False), N=4133, n=64, d=128)
    add("qmc-heston-bridge-n252-seedA-N100", "olmc_heston_qmc", "sobol bridge slabs ws", lambda: h.heston_qmc(QS, QK, QT, QR, HQ, True, *HESTON, 100, *tables(504, SEED_A), True, False), N=100, n=252, d=504)
    add("qmc-heston-paths-bridge-n64-seedA-N257", "olmc_heston_qmc_paths", "sobol bridge slabs bulk", lambda: h.heston_qmc_paths(QS, QT, QR, HQ, *HESTON, 257, *tables(128, SEED_A), True, True), N=514, n=64, d=128)
    add("qmc-heston-paths-sequential-n13-seedA-N100", "olmc_heston_qmc_paths", "sobol bulk", lambda: h.heston_qmc_paths(QS, QT, QR, HQ, *HESTON, 100, *tables(26, SEED_A), False, False), N=200, n=13, d=26)
    add("qmc-heston-path-payoff-bridge-n64-seedB-N257", "olmc_heston_qmc_path_payoff", "sobol bridge slabs ws",
        lambda: h.heston_qmc_path_payoff(QS, QK, QT, QR, HQ, True, *HESTON, BARRIER_UP_OUT, UP, 257, *tables(128, SEED_B), True, False), N=257, n=64, d=128)
    add("qmc-heston-surface-bridge-n13-seedA-N4133", "olmc_heston_qmc_surface", "sobol bridge slabs ws ws_wide",
        lambda: h.heston_qmc_surface(QS, QT, QR, HQ, True, *HESTON, *_cells(13), 4133, *tables(26, SEED_A), True, False), N=4133, n=13, d=26, k=3)
    add("qmc-heston-scenarios-bridge-n5-seedA-N257", "olmc_heston_qmc_scenarios", "sobol bridge slabs ws ws_wide",
        lambda: h.heston_qmc_scenarios(_scenario_set(), 257, *tables(10, SEED_A), True, True), N=257, n=5, d=10, k=4)
    add("qmc-heston-greeks-bridge-second-n13-seedB-N100", "olmc_heston_qmc_greeks_fd", "sobol bridge slabs ws ws_wide",
        lambda: h.heston_qmc_greeks_fd(*QEURO, True, *HESTON[:4], 100, *tables(26, SEED_B), True, False, True), N=100, n=13, d=26, k=14)
    add("qmc-heston-qe-surface-n64-seedA-N257", "olmc_heston_qe_qmc_surface", "sobol ws ws_wide",
        lambda: h.heston_qe_qmc_surface(QS, QT, QR, HQ, False, *HESTON, *_cells(64), 257, *tables(128, SEED_A), False, True), N=257, n=64, d=128, k=3)
    add("qmc-heston-qe-paths-n13-seedA-N100", "olmc_heston_qe_qmc_paths", "sobol bulk", lambda: h.heston_qe_qmc_paths(QS, QT, QR, HQ, *HESTON, 100, *tables(26, SEED_A), False, True), N=200, n=13, d=26)
    add("qmc-heston-autocallable-euler-bridge-n64-seedA-N100", "olmc_heston_autocallable_qmc", "sobol bridge slabs ws",
        lambda: h.heston_autocallable_qmc(QS, QT, QR, HQ, *HESTON, *AUTOCALL, OBS[64], 100, *tables(128, SEED_A), True, False), N=100, n=64, d=128)
    add("qmc-heston-autocallable-qe-n64-seedA-N100", "olmc_heston_autocallable_qmc", "sobol ws",
        lambda: h.heston_autocallable_qmc(QS, QT, QR, HQ, *HESTON, *AUTOCALL, OBS[64], 100, *tables(128, SEED_A), False, False, qe=True), N=100, n=64, d=128)
    add("qmc-heston-cliquet-euler-bridge-n13-seedA-N257", "olmc_heston_cliquet_qmc", "sobol bridge slabs ws",
        lambda: h.heston_cliquet_qmc(QS, QT, QR, HQ, *HESTON, *CLIQUET, PER[13], 257, *tables(26, SEED_A), True, True), N=257, n=13, d=26)
    add("qmc-heston-cliquet-qe-n5-seedA-N100", "olmc_heston_cliquet_qmc", "sobol ws",
        lambda: h.heston_cliquet_qmc(QS, QT, QR, HQ, *HESTON, *CLIQUET, PER[5], 100, *tables(10, SEED_A), False, False, qe=True), N=100, n=5, d=10)

    # ---- single-process multi-GPU entry points on one rank (the rank's own context)
    add("multi-gpu-european-N4133-n13", "olmc_multi_gpu_european", "ws", lambda: h.multi_gpu_european(*EURO, True, 4133, 13, SEED, True, 1), N=4133, n=13)
    add("multi-gpu-greeks-second-N257-n5", "olmc_multi_gpu_greeks_fd", "ws ws_wide", lambda: h.multi_gpu_greeks_fd(*EURO, True, 257, 5, SEED, True, 1), N=257, n=5, k=14)
    add("multi-gpu-cv-N257-n13", "olmc_multi_gpu_european_cv", "ws ws_wide", lambda: h.multi_gpu_european_cv(*EURO, False, 257, 13, SEED, True, 1), N=257, n=13, k=5)
    add("multi-gpu-qmc-d64-seedB-N4133", "olmc_multi_gpu_european_qmc", "sobol ws", lambda: h.multi_gpu_european_qmc(*QEURO, True, 4133, *tables(64, SEED_B), 1), N=4133, d=64)
    add("multi-gpu-qmc-greeks-first-d13-seedA-N257", "olmc_multi_gpu_european_qmc_greeks_fd", "sobol ws ws_wide",
        lambda: h.multi_gpu_european_qmc_greeks_fd(*QEURO, False, 257, *tables(13, SEED_A), False, 1), N=257, d=13, k=8)
    add("multi-gpu-qmc-cv-d5-seedA-N100", "olmc_multi_gpu_european_qmc_cv", "sobol ws ws_wide", lambda: h.multi_gpu_european_qmc_cv(*QEURO, True, 100, *tables(5, SEED_A), 1), N=100, d=5, k=5)
    return out


# what the catalogue does not call, and why (tests/test_call_catalogue_cpu.py holds the header to catalogue + this table)
EXEMPT = {
    "olmc_abi_version": "a constant",
    "olmc_init": "lifetime: the history test's own fresh start",
    "olmc_shutdown": "lifetime: the history test's own fresh start",
    "olmc_last_error": "the calling thread's message, no device state",
    "olmc_device_info": "device properties, computes nothing",
    "olmc_contract_layout": "host arithmetic only",
    "olmc_multi_capacity": "reads the batch workspace's size, computes nothing",
    "olmc_heston_scenario_layout": "host arithmetic only",
    "olmc_combine_cv": "host arithmetic only",
    "olmc_combine_stats": "host arithmetic only",
    "olmc_multi_gpu_spans": "host timings of the last call",
    "olmc_tune": "a switch: the history test toggles it around the catalogue's calls",
    "olmc_profile_enable": "a switch: the history test toggles it around the catalogue's calls",
    "olmc_profile_reset": "measurement bookkeeping",
    "olmc_kernel_time": "measurement bookkeeping",
}
# olmc_philox_words and olmc_normals are CATALOGUED, not exempt: they are validation taps, but they launch on context 0 and stage their
# output in the bulk buffer, after and before every path matrix -- the parity tests' oracle for the stream itself reads through it.
