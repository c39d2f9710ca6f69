"""The local-volatility entry points give the bits of a freshly initialised library whatever ran before them.

tests/test_gpu_call_history.py's bar for include/olmc_local_vol.h: the BASELINE of a call is the same call as the first one after
olmc_shutdown (the next call initialises a new library), results are compared as uint64 words (call_catalogue.words), and once a call
fails unexpectedly nothing more is started on the device.  What a context keeps for this family is the device copy of the table (a
buffer of the caps' size, rewritten by every call) and what every reducing or matrix call keeps (workspace, bulk buffer).  Each of the
three entry points runs after
  (a) the same entry point with a larger table (the caps, 64 x 256), then with a smaller one (1 x 2): old nodes must not show through;
  (b) an olmc_heston_qmc bridge call (Sobol table, bridge plan and slabs on the same context);
  (c) a refused ollv_price (an argument error, made before any device work).
"""
import pytest

from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import call_catalogue as cc
from tests import test_gpu_local_vol as lv
from tests.history import Device, baseline_fixture, check_fresh_bits_after

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

N, STEPS = 257, 13
CELLS = ([95.0, 105.0, 100.0], [13, 4, 5])
DEVICE = Device()


def calls(name):
    """The three entry points on table `name` of tests/test_gpu_local_vol.py."""
    table = lv.TABLES[name].args
    return {
        "ollv_price": lambda: [_hip.lv_price(lv.S, lv.K, lv.T, lv.R, lv.Q, True, table, code, level, N, STEPS, lv.SEED, True)
                               for code, level in ((0, lv.UP), (6, 0.0), (lv.EUROPEAN, 0.0))],
        "ollv_paths": lambda: _hip.lv_paths(lv.S, lv.T, lv.R, lv.Q, table, N, STEPS, lv.SEED, path_major=True),
        "ollv_surface_prices": lambda: _hip.lv_surface_prices(lv.S, lv.T, lv.R, lv.Q, False, table, *CELLS, N, STEPS, lv.SEED, True),
    }


def refused_price():
    with pytest.raises(AccelerationError, match="bad payoff"):
        _hip.lv_price(lv.S, lv.K, lv.T, lv.R, lv.Q, True, lv.TABLES["33x128"].args, 9, 0.0, N, STEPS, lv.SEED)
    return 0


baseline = baseline_fixture(DEVICE, lambda: calls("33x128"))


HISTORIES = {
    "larger-then-smaller-table": lambda entry: [calls("64x256")[entry], calls("1x2")[entry]],
    "heston-qmc-bridge": lambda entry: [{e.name: e for e in cc.catalogue()}["qmc-heston-bridge-n13-seedA-N257"].call],
    "refused-price": lambda entry: [refused_price],
}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("entry", ["ollv_price", "ollv_paths", "ollv_surface_prices"])
def test_entry_point_gives_the_fresh_library_s_bits_after(baseline, entry, history):
    check_fresh_bits_after(DEVICE, baseline, entry, calls("33x128")[entry], history, HISTORIES[history](entry))
