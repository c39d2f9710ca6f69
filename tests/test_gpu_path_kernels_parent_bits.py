"""The path kernels give, word for word, what they gave before their pieces were shared.

tests/golden/path_kernels_parent_bits.json (generator: tests/golden/make_path_kernels_parent_bits.py) was recorded on the commit before
the surface prologue, the wave-uniform Philox path loop, the local-volatility step walk and the host runners of these entry points
were written once (the price kernels' payoff tail, which stayed written out, is covered all the same).  Every call of tests/path_kernels_calls.py is repeated here and compared with the fixture:
the uint64 words of (sum, sumsq) and n of every Stats; of every matrix the shape, the sha256 of all its words and, path-major, its first
and last rows.  The same module passes on the commit that recorded the fixture (through $OLMC_LIBRARY).  As in the history tests, once a
call fails unexpectedly nothing more is started on the device.
"""
import json
import os

import pytest

from optionslab_amd import _hip
from tests import path_kernels_calls as pk
from tests.history import Device

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_kernels_parent_bits.json")
DEVICE = Device(record=lambda words: words)             # pk.record takes the label: the calls below record themselves


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert (doc["S"], doc["K"], doc["T"], doc["r"], doc["q"], doc["sigma"], doc["seed"], doc["table"]) == (pk.S, pk.K, pk.T, pk.R, pk.Q, pk.SIGMA, pk.SEED, pk.TABLE)
    assert set(doc["shapes"]) == set(pk.SHAPES)
    return doc["shapes"]


@pytest.mark.parametrize("group", pk.GROUPS)
@pytest.mark.parametrize("shape", list(pk.SHAPES))
def test_every_call_gives_the_parent_commit_s_words(golden, shape, group):
    N, n, cap = pk.SHAPES[shape]
    want = golden[shape][group]
    calls = pk.calls(group, N, n)
    assert set(calls) == set(want) and len(calls) > 0
    _hip.tune(_hip.TUNE_GRID_CAP, cap)
    try:
        got = {label: DEVICE.invoke(label, lambda: pk.record(label, call())) for label, call in calls.items()}
    finally:
        _hip.tune(_hip.TUNE_GRID_CAP, 0)                        # the knob is process-global: 0 again whatever happens
    differ = [label for label in calls if got[label] != want[label]]
    for label in differ[:4]:
        print(label, "got", got[label], "want", want[label])
    assert not differ, f"{shape} {group}: {len(differ)} of {len(calls)} calls differ from the parent commit's words: {differ[:8]}"
