#!/usr/bin/env python3
"""Generate tests/golden/path_kernels_parent_bits.json by RUNNING the calls of tests/path_kernels_calls.py on the device.

    python tests/golden/make_path_kernels_parent_bits.py [output.json]

Run it on the commit BEFORE the path kernels' surface prologue, Philox path loop and local-volatility walk were shared (or on
any later one: the point of the fixture is that the answer is the same; $OLMC_LIBRARY names another build of the library).  It records,
for every call of every group at both shapes, the uint64 words of (sum, sumsq) and n of each Stats, and of a matrix the sha256 of its
little-endian bytes (equal digests are equal words, every one of them) plus, path-major, its first and last rows, so that a mismatch
says more than a digest does.  The fixture holds numbers only.
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "path_kernels_parent_bits.json")


def main():
    from optionslab_amd import _hip
    from tests import path_kernels_calls as pk

    warnings.filterwarnings("ignore", message="The balance properties of Sobol")
    shapes = {}
    for shape, (N, n, cap) in pk.SHAPES.items():
        _hip.tune(_hip.TUNE_GRID_CAP, cap)
        try:
            shapes[shape] = {group: {label: pk.record(label, call()) for label, call in pk.calls(group, N, n).items()} for group in pk.GROUPS}
        finally:
            _hip.tune(_hip.TUNE_GRID_CAP, 0)
        print(shape, {group: len(docs) for group, docs in shapes[shape].items()})
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(generator="tests/golden/make_path_kernels_parent_bits.py", S=pk.S, K=pk.K, T=pk.T, r=pk.R, q=pk.Q, sigma=pk.SIGMA, seed=pk.SEED,
                       table=pk.TABLE, shapes=shapes), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
