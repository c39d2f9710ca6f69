"""Plain reference of the synthetic values olmc_reduce_probe feeds the fused grid reduction (tools/probe/olmc_probe_kernels.h), in
integer arithmetic: NumPy uint64 masked to 32 bits for the hashes, Python int for the totals.

Thread t of workgroup b contributes to component c
    v = H(b, c, salt) + K(t, c, salt)        when 256 b + t < n_threads, else 0
with (all mod 2^32)
    mix32(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
    seed = mix32(lo32(salt) ^ mix32(hi32(salt) ^ 0x9E3779B9))
    H    = (mix32( seed + b * 0x9E3779B1 + c * 0x85EBCA6B) >>  8) | 1       24 bits, odd
    K    = (mix32(~seed + t * 0xC2B2AE35 + c * 0x27D4EB2F) >> 16) | 1       16 bits, odd
The form is separable on purpose: with live(b) threads alive in workgroup b and count(t) workgroups in which thread t is alive,
    total(c) = sum_b live(b) H(b, c) + sum_t count(t) K(t, c),
which is G + 256 hash evaluations per component instead of n_threads.  At most 2^26 threads x (2^24 + 2^16) < 2^51: every partial sum
of the device's fp64 additions is an exact integer whatever their order, so the device total must EQUAL total(c).

values = 1 of the tap divides each thread's integer by 3.0 (one correctly rounded fp64 division): `rounded_values` are those doubles."""
import math

import numpy as np

BLOCK = 256
MAX_WORKGROUPS = 1 << 18
_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix32(x):
    x = _u64(x) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def seed32(salt):
    salt = int(salt)
    return mix32((salt & 0xFFFFFFFF) ^ int(mix32(((salt >> 32) & 0xFFFFFFFF) ^ 0x9E3779B9)))


def hash_h(b, c, salt):
    """24-bit odd hash of (workgroup, component): uint64 array of the broadcast shape of b and c."""
    x = (seed32(salt) + _u64(b) * np.uint64(0x9E3779B1) + _u64(c) * np.uint64(0x85EBCA6B)) & _M32
    return (mix32(x) >> np.uint64(8)) | np.uint64(1)


def hash_k(t, c, salt):
    """16-bit odd hash of (thread, component)."""
    x = ((seed32(salt) ^ _M32) + _u64(t) * np.uint64(0xC2B2AE35) + _u64(c) * np.uint64(0x27D4EB2F)) & _M32
    return (mix32(x) >> np.uint64(16)) | np.uint64(1)


# ---- the same, one value at a time, in Python integers (what the vectorised forms are tested against)
def mix32_scalar(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def seed32_scalar(salt: int) -> int:
    return mix32_scalar((salt & 0xFFFFFFFF) ^ mix32_scalar(((salt >> 32) & 0xFFFFFFFF) ^ 0x9E3779B9))


def hash_h_scalar(b: int, c: int, salt: int) -> int:
    return (mix32_scalar(seed32_scalar(salt) + b * 0x9E3779B1 + c * 0x85EBCA6B) >> 8) | 1


def hash_k_scalar(t: int, c: int, salt: int) -> int:
    return (mix32_scalar((seed32_scalar(salt) ^ 0xFFFFFFFF) + t * 0xC2B2AE35 + c * 0x27D4EB2F) >> 16) | 1


def workgroups(n_threads: int) -> int:
    return (int(n_threads) + BLOCK - 1) // BLOCK


def expected(nv: int, n_threads: int, salt: int) -> list:
    """[total(c) for c < nv] as Python integers, by the separable closed form."""
    n = int(n_threads)
    full, rem = divmod(n, BLOCK)
    g = workgroups(n)
    if not 1 <= g <= MAX_WORKGROUPS:
        raise ValueError("n_threads outside one launch")
    c = np.arange(nv, dtype=np.uint64)[None, :]
    live = np.full(g, BLOCK, dtype=np.uint64)
    if rem:
        live[-1] = rem
    count = np.full(BLOCK, full, dtype=np.uint64)
    count[:rem] += np.uint64(1)
    h = hash_h(np.arange(g, dtype=np.uint64)[:, None], c, salt)           # [g, nv], < 2^24
    k = hash_k(np.arange(BLOCK, dtype=np.uint64)[:, None], c, salt)       # [256, nv], < 2^16
    sums = (live[:, None] * h).sum(axis=0, dtype=np.uint64) + (count[:, None] * k).sum(axis=0, dtype=np.uint64)     # < 2^51: no wrap
    return [int(s) for s in sums]


def thread_values(nv: int, n_threads: int, salt: int) -> np.ndarray:
    """The integers of every live thread, [n_threads, nv] uint64 (brute force: small n_threads only)."""
    i = np.arange(int(n_threads), dtype=np.uint64)
    c = np.arange(nv, dtype=np.uint64)[None, :]
    return hash_h((i // np.uint64(BLOCK))[:, None], c, salt) + hash_k((i % np.uint64(BLOCK))[:, None], c, salt)


def rounded_values(nv: int, n_threads: int, salt: int) -> np.ndarray:
    """values = 1: double(H + K) / 3.0 of every live thread, [n_threads, nv] float64."""
    return thread_values(nv, n_threads, salt).astype(np.float64) / 3.0


def rounded_reference(nv: int, n_threads: int, salt: int):
    """(fsum, sum |v|, number of addends) per component of the values = 1 doubles: fsum is their correctly rounded sum."""
    v = rounded_values(nv, n_threads, salt)
    return [math.fsum(v[:, c]) for c in range(nv)], [math.fsum(np.abs(v[:, c])) for c in range(nv)], v.shape[0]


# ---- the launch shapes of tests/test_gpu_reduction.py (the CPU test checks that every total they lead to stays exact)
# 10 and 22 are HaBasis<1>::NV and HaBasis<2>::NV (the Heston American fit); HaBasis<3>::NV = 39 is wider than a workspace row of the grid
# reduction (32 values) and exists in the hand-over form alone (below)
NV_FORMS = [(nv, form) for nv in (2, 5, 8, 10, 16, 22, 32) for form in (0, 1, 2) if form != 1 or nv >= 8]
# one group; a group of exactly 256; a second group of one workgroup; the SUBS and SUBS * kBatch boundaries of every padded width
SWEEP_G = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000)
BIG_G = (65_537, 1 << 18)               # 257 groups (second trip of the level-2 row sum); the largest grid (1,024 groups)
SEQUENCE_G = (700, 1, 257, 256, 1000, 3, 513, 65_537)       # several groups, one group, many again: counters must come back to zero
SEQUENCE_LAUNCHES = 64


def sweep_threads() -> list:
    """n_threads of the shape sweep: every G full, with one thread in the last workgroup, and with one thread missing."""
    return [n for g in SWEEP_G for n in (BLOCK * g, BLOCK * g - (BLOCK - 1), BLOCK * g - 1)]


def sweep_salts(nv: int, form: int, blocking: int) -> list:
    """A salt per launch of the sweep, different for every (nv, form, blocking); some above 2^32."""
    return [(nv << 40) ^ (form << 36) ^ (blocking << 34) ^ (0x9E3779B97F4A7C15 * (j + 1) & 0xFFFFFFFFFF) for j in range(len(sweep_threads()))]


def sequence(nv: int):
    """(n_threads, salts) of the 64 back-to-back launches: grid sizes cycle through SEQUENCE_G (every other launch with a ragged last
    workgroup), all salts different."""
    n = [BLOCK * SEQUENCE_G[j % len(SEQUENCE_G)] - (0 if (j + j // 8) % 2 == 0 else 1 + (37 * j) % 255) for j in range(SEQUENCE_LAUNCHES)]
    salts = [(nv << 48) + 0x1_0000_0001 * (j + 1) for j in range(SEQUENCE_LAUNCHES)]
    return n, salts


def big_launches():
    """(n_threads, salts) of the launches past 65,536 workgroups: each BIG_G full, and with one thread in its last workgroup."""
    n = [x for g in BIG_G for x in (BLOCK * g, BLOCK * g - (BLOCK - 1))]
    return n, [0x5_0000_0000 + j for j in range(len(n))]


# ---- form 3, the hand-over of the LSM chains: G1 workgroups store block_row_sum<nv> rows, G2 workgroups each sum all of them by
# workgroup_rows_sum<nv>.  The widths are kLsmNV and HaBasis<D>::NV; the chains launch at most 1,024 workgroups.
HAND_OVER_NV = (16, 10, 22, 39)
HAND_OVER_G1 = (1, 2, 255, 256, 257, 1024)
HAND_OVER_G2 = (1, 3, 256)


def padded_width(nv: int, whole_workgroup: bool) -> int:
    """NVP of workgroup_rows_sum<nv> (8, 16, 32, 64: the 39 sums of degree 3 take a whole wave's width) / wave_rows_sum<nv> (2, 8, 16, 32)."""
    if whole_workgroup:
        return 8 if nv <= 8 else 16 if nv <= 16 else 32 if nv <= 32 else 64
    return 2 if nv <= 2 else 8 if nv <= 8 else 16 if nv <= 16 else 32


def subs_batch(nv: int, whole_workgroup: bool):
    """(SUBS, kBatch): row subsets per column and loads in flight per lane; NVP = 64 gives (4, 16)."""
    nvp = padded_width(nv, whole_workgroup)
    if whole_workgroup:
        return BLOCK // nvp, 16 if nvp >= 16 else 8
    return 64 // nvp, 8


def transpose_width(nv: int) -> int:
    """P of block_row_sum<nv>: nv padded to a power of two (39 -> 64: SHIFT = 0, a value index per lane)."""
    p = 1
    while p < nv:
        p *= 2
    return p


def hand_over_launches(nv: int):
    """(n_threads, salts) of form 3's first launches: every G1 full, with one thread in the last workgroup, and with one thread missing."""
    n = [x for g in HAND_OVER_G1 for x in (BLOCK * g, BLOCK * g - (BLOCK - 1), BLOCK * g - 1)]
    return n, [(nv << 44) ^ (0xC2B2AE3D27D4EB4F * (j + 1) & 0xFFFFFFFFFFF) for j in range(len(n))]
