"""The European kernels' one-sine pair sums against the device's own individual normals (run with `-m gpu`).

european_path_kernel sums a path's normals in pair-sum units (olmc_kernels.h, "Pair sums"): whole pairs as rad * sin(turns + 1/8),
in the partial block a first pair the same way and an odd leftover normal times 1 / sqrt(2), and the path's sum scaled by
2 sqrt(ln 2).  olmc_normals still returns every normal on its own (rad * cos, rad * sin).  Rebuilding the terminal prices in fp64
from those normals on the same seed checks the bookkeeping of every n_steps % 4 and of an odd leftover: a unit that is off by
sqrt(2) on one normal moves a price by ~1e-2 relative, far above what fp32 rounding and the hardware sine leave (~1e-7).

This is the bookkeeping only: REL lets through anything a hundred times the chain's rounding.  The chain itself -- every fma, the
association of the groups and quarters, the constants -- is pinned bit for bit by tests/normal_sum_oracle.py, against which
tests/test_gpu_normal_sums_exact.py holds the same kernels at fp64's own scale."""
import math

import numpy as np
import pytest

from optionslab_amd import _hip
from tests.gpu_support import device_fixture

pytestmark = pytest.mark.gpu

S, T, R, V, Q = 100.0, 1.0, 0.05, 0.2, 0.01
SEED = 2024
N = 4096
REL = 2e-6        # fp32 partial sums and hardware transcendentals on the normal sum, times vol <= 0.2


_device = device_fixture()


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 252, 253])
def test_terminal_prices_equal_the_ones_rebuilt_from_individual_normals(M):
    got = _hip.european_terminal(S, T, R, V, Q, N, M, SEED, True)
    z = _hip.normals(SEED, 0, N, M).astype(np.float64)
    zsum = z.sum(axis=1)
    a = math.log(S) + (R - Q - 0.5 * V * V) * T
    vol = V * math.sqrt(T / M)
    want = np.concatenate([np.exp(a + vol * zsum), np.exp(a - vol * zsum)])
    assert got.shape == want.shape and np.isfinite(got).all()
    rel = np.abs(got / want - 1.0)
    assert rel.max() <= REL, (M, float(rel.max()), int(rel.argmax()))
