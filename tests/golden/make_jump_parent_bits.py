#!/usr/bin/env python3
"""Generate tests/golden/jump_parent_bits.json by RUNNING olmc_jump_diffusion and olmc_jump_paths on the device.

    python tests/golden/make_jump_parent_bits.py [output.json]

Run it on the commit BEFORE include/olmc_jump.h existed (or on any later one: the point of the fixture is that the answer is the same).
It records, for the four jump models of tests/test_gpu_jump_payoffs.py at (N, n) in {(257, 13), (1000, 2), (4097, 64)} with seed 17,
the uint64 words of
  - olmc_jump_diffusion's (sum, sumsq), call and put, and
  - olmc_jump_paths' matrix in both layouts: the sha256 of its little-endian bytes (equal digests are equal words, every one of them), and
    path-major also its first and last rows, so that a mismatch says more than a digest does.
The fixture holds numbers only.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "jump_parent_bits.json")

S, K, T, R, Q, SIGMA, SEED = 100.0, 100.0, 1.0, 0.05, 0.01, 0.2, 17
SHAPES = ((257, 13), (1000, 2), (4097, 64))
# (name, kou, lambda_j, a1, a2, a3)
MODELS = (("M0", False, 0.5, -0.1, 0.2, 0.0), ("M1", False, 40.0, 0.02, 0.1, 0.0), ("K0", True, 1.0, 0.4, 10.0, 5.0), ("K1", True, 60.0, 0.6, 25.0, 20.0))


def hex_words(a):
    """The uint64 words of the doubles, 16 hex digits each, separated by blanks."""
    return " ".join("%016x" % int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel())


def matrix_record(m, path_major):
    m = np.ascontiguousarray(m, dtype=np.float64)
    raw = m.astype("<f8").tobytes()
    doc = dict(shape=list(m.shape), sha256=hashlib.sha256(raw).hexdigest())
    if path_major:                                           # a row is a path: n_steps + 1 words
        doc.update(first_row=hex_words(m[0]), last_row=hex_words(m[-1]))
    return doc


def main():
    from optionslab_amd import _hip

    cases = []
    for n_paths, n_steps in SHAPES:
        for name, kou, lam, a1, a2, a3 in MODELS:
            doc = dict(model=name, n_paths=n_paths, n_steps=n_steps)
            if lam * T / n_steps > 20.0:                     # K1 at two steps: 30 jumps per step, which both entry points refuse
                for label, call in (("price", lambda: _hip.jump_diffusion(S, K, T, R, SIGMA, Q, True, kou, lam, a1, a2, a3, n_paths, n_steps, SEED)),
                                    ("paths", lambda: _hip.jump_paths(S, T, R, SIGMA, Q, kou, lam, a1, a2, a3, n_paths, n_steps, SEED))):
                    try:
                        call()
                        raise SystemExit(f"{name} {n_paths} x {n_steps}: {label} was expected to be refused")
                    except _hip.AccelerationError as e:
                        doc["refused_" + label] = str(e)
                cases.append(doc)
                print(f"{name} {n_paths} x {n_steps}: refused ({doc['refused_price']})")
                continue
            for is_call in (True, False):
                st = _hip.jump_diffusion(S, K, T, R, SIGMA, Q, is_call, kou, lam, a1, a2, a3, n_paths, n_steps, SEED)
                doc["call" if is_call else "put"] = dict(sums=hex_words([st.sum, st.sumsq]), n=int(st.n))
            for path_major in (True, False):
                m = _hip.jump_paths(S, T, R, SIGMA, Q, kou, lam, a1, a2, a3, n_paths, n_steps, SEED, path_major=path_major)
                doc["path_major" if path_major else "step_major"] = matrix_record(m, path_major)
            cases.append(doc)
            print(f"{name} {n_paths} x {n_steps}: call sums {doc['call']['sums']}")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(generator="tests/golden/make_jump_parent_bits.py", S=S, K=K, T=T, r=R, q=Q, sigma=SIGMA, seed=SEED, cases=cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
