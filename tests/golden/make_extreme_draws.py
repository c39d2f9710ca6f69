#!/usr/bin/env python3
"""Generate tests/golden/extreme_draws.json: global paths whose FIRST Philox block holds an extreme radius word.

    python tests/golden/make_extreme_draws.py          # about 20 s per seed

A radius word below 128 (u_a < 2^-25: a normal beyond 5.8 sigma) or at least 0xFFFFFF80 (u_a rounds to 1: two normals that are exact
zeros) turns up once in 2^24 words, so no seeded test ever draws one.  This script scans paths 0 .. 2^26 - 1 of seeds 42 and 7 at
block 0 with the NumPy Philox of tests/box_muller_reference.py, looks at the two radius words x0 (steps 0, 1) and x2 (steps 2, 3), and
records every hit as (seed, path, word slot, word).  tests/test_box_muller_cpu.py checks each entry against the C checker's Philox,
tests/test_gpu_box_muller.py against the device's and then prices those very paths with n_paths = 1.  Numbers only.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "extreme_draws.json")
SEEDS, LOG2_PATHS, CHUNK = (42, 7), 26, 1 << 21


def main():
    sys.path.insert(0, ROOT)
    from tests import box_muller_reference as bm

    entries = []
    for seed in SEEDS:
        for lo in range(0, 1 << LOG2_PATHS, CHUNK):
            words = bm.philox_words(seed, np.arange(lo, lo + CHUNK, dtype=np.uint64))
            for slot in (0, 2):
                x = words[:, slot]
                for i in np.flatnonzero((x < bm.TAIL_WORDS) | (x >= bm.ONE_WORDS)):
                    entries.append(dict(seed=seed, path=lo + int(i), slot=slot, word=int(x[i]), kind="tail" if x[i] < bm.TAIL_WORDS else "one"))
    entries.sort(key=lambda e: (e["kind"], e["seed"], e["path"], e["slot"]))
    kinds = [e["kind"] for e in entries]
    assert kinds.count("tail") >= 4 and kinds.count("one") >= 4, kinds
    doc = dict(comment="paths whose block 0 holds a radius word < 128 ('tail') or >= 0xFFFFFF80 ('one'); slot 0 = x0 (steps 0, 1), "
                       "slot 2 = x2 (steps 2, 3); made by make_extreme_draws.py",
               seeds=list(SEEDS), block=0, paths_scanned=1 << LOG2_PATHS, entries=entries)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(entries)} entries ({kinds.count('tail')} tail, {kinds.count('one')} one) -> {OUT}")


if __name__ == "__main__":
    main()
