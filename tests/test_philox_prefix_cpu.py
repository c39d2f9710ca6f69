"""philox_prefix (optionslab_amd/csrc/olmc_host_math.h): the three words per Philox block that every path of a European launch shares
after two rounds, built by the host once per launch.  The header is compiled on its own (tests/philox_prefix_harness.cpp, g++ with
AddressSanitizer + UBSan where the runtime is installed) and held against the checker's generator, oracle/philox_oracle.py: a
restatement of ONE Philox round here is first tied to the checker (ten of them are its philox()), then the table words must be the
words that round gives after rounds 1 and 2, and rounds 3-10 continued from the table words and the path's own words must end in
the checker's ten-round output."""
import os
import random
import shutil
import subprocess

import pytest

from oracle import philox_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox_round(c, k):
    """One round of Philox4x32 (Salmon et al., SC'11): the new counter; the caller bumps the key."""
    p0, p1 = M0 * c[0], M1 * c[2]
    return [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]


def bump(k):
    return [(k[0] + W0) & MASK, (k[1] + W1) & MASK]


def rounds(c, k, n):
    for _ in range(n):
        c, k = philox_round(c, k), bump(k)
    return c, k


@pytest.fixture(scope="module")
def table_words(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("philox_prefix") / "philox_prefix"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "optionslab_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "philox_prefix_harness.cpp")]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        build = subprocess.run(base, capture_output=True, text=True)          # no sanitizer runtime here: the plain program
    assert build.returncode == 0, build.stderr

    def run(cases):
        """cases: (seed, g_hi, tag, n_blocks, block) -> (n_blocks, [w0, w1, w2, w3], stray non-zero words)"""
        text = "".join(" ".join(str(int(x)) for x in case) + "\n" for case in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return [(row[0], row[1:5], row[5]) for row in rows]

    return run


def random_cases(n=200):
    rng = random.Random(20260)
    edge = [0, 1, MASK, 0x80000000]
    cases = []
    for i in range(n):
        word = lambda: rng.choice(edge) if rng.random() < 0.15 else rng.getrandbits(32)
        seed = rng.choice([0, 42, (1 << 64) - 1, 7 << 32]) if rng.random() < 0.15 else rng.getrandbits(64)
        block = (0, 1, 62, 63)[i] if i < 4 else rng.randrange(64)
        cases.append(dict(seed=seed, g_hi=word(), tag=word(), g_lo=word(), block=block, n_blocks=rng.choice([64, block + 1])))
    return cases


def test_the_round_restated_here_is_the_checkers_generator():
    for c in random_cases(50):
        ctr, key = [c["g_lo"], c["g_hi"], c["block"], c["tag"]], [c["seed"] & MASK, c["seed"] >> 32]
        assert rounds(ctr, key, 10)[0] == po.philox(ctr, key)


def test_table_words_are_the_shared_words_after_rounds_one_and_two_and_continue_to_the_checkers_output(table_words):
    cases = random_cases(200)
    got = table_words([(c["seed"], c["g_hi"], c["tag"], c["n_blocks"], c["block"]) for c in cases])
    for c, (n_blocks, w, stray) in zip(cases, got):
        assert n_blocks == c["n_blocks"] and stray == 0 and w[3] == 0
        ctr, key = [c["g_lo"], c["g_hi"], c["block"], c["tag"]], [c["seed"] & MASK, c["seed"] >> 32]
        s1, k1 = rounds(ctr, key, 1)
        s2, k2 = rounds(s1, k1, 1)
        # the three shared words, read off the state after round 1 and after round 2
        assert w[0] == s1[1]                                   # lo(M1 b)
        assert w[1] == s2[2] ^ s1[3] ^ k1[1]                   # hi(M0 c0'): c2 of round 2 without the path's lo(M0 g_lo) and the key
        assert w[2] == s2[3]                                   # lo(M0 c0')
        # the path's own words, from the path alone (no block, no g_hi, no low key word): c2' and lo(M0 g_lo)
        p0 = M0 * c["g_lo"]
        c2_1 = (p0 >> 32) ^ c["tag"] ^ key[1]
        p1 = M1 * c2_1
        lane_a, lane_b, lane_c = (p1 >> 32) ^ k1[0], (p0 & MASK) ^ k1[1], p1 & MASK
        state = [lane_a ^ w[0], lane_c, lane_b ^ w[1], w[2]]   # what the kernel forms per block: two 2-input XORs
        assert state == s2
        assert rounds(state, k2, 8)[0] == po.philox(ctr, key)  # rounds 3-10 from there: the checker's ten-round output


def test_the_count_is_clamped_to_the_capacity(table_words):
    got = table_words([(42, 0, 0, 70, 63), (42, 0, 0, 0, 0), (42, 0, 0, -3, 5)])
    assert [g[0] for g in got] == [64, 0, 0]
    assert got[1][1] == [0, 0, 0, 0] and got[2][1] == [0, 0, 0, 0] and all(g[2] == 0 for g in got)
