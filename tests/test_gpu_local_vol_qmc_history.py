"""The olvq_* entry points give the bits of a freshly initialised library whatever ran before them.

tests/test_gpu_local_vol_history.py's bar for include/olmc_local_vol_qmc.h: the BASELINE of a call is the same call as the first one
after olmc_shutdown, results are compared as uint64 words (call_catalogue.words), and once a call fails unexpectedly nothing more is
started on the device.  What a context keeps for this family: the device copy of the table, the Sobol tables and the bridge plan of the
last call, and the bridge slabs it shares with the Heston Sobol kernels.  Each of the three entry points (bridge, 257 x 13 on "33x128")
runs after
  (a) the same entry point with the caps' 64 x 256 table, then with the 1 x 2 one: old nodes must not show through;
  (b) the catalogue's olmc_heston_qmc bridge call at 13 steps (the Sobol table, plan and slabs of the same context, laid out for two
      factors), then the same entry point at n = 64 with another seed (larger tables, another plan, larger slabs);
  (c) a Philox ollv_price (the table uploaded in units of the raw normals);
  (d) a refused olvq_price (an argument error, made before any device work).
"""
import pytest

from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import call_catalogue as cc
from tests import test_gpu_local_vol as lv
from tests.history import Device, baseline_fixture, check_fresh_bits_after

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

N, STEPS = 257, 13
ENTRIES = ["olvq_price", "olvq_paths", "olvq_surface_prices"]
DEVICE = Device()


def cells(n):
    return [95.0, 105.0, 100.0], [n, 4, 5]


def calls(name, n=STEPS, seed=cc.SEED_A):
    """The three entry points, bridge, on table `name` of tests/test_gpu_local_vol.py."""
    table = lv.TABLES[name].args
    tables = lambda: cc.tables(n, seed)
    return {
        "olvq_price": lambda: [_hip.lvq_price(lv.S, lv.K, lv.T, lv.R, lv.Q, True, table, code, level, N, *tables(), True, True)
                               for code, level in ((0, lv.UP), (6, 0.0), (lv.EUROPEAN, 0.0))],
        "olvq_paths": lambda: _hip.lvq_paths(lv.S, lv.T, lv.R, lv.Q, table, N, *tables(), True, path_major=True),
        "olvq_surface_prices": lambda: _hip.lvq_surface_prices(lv.S, lv.T, lv.R, lv.Q, False, table, *cells(n), N, *tables(), True, True),
    }


def philox_price():
    return _hip.lv_price(lv.S, lv.K, lv.T, lv.R, lv.Q, True, lv.TABLES["64x256"].args, 6, 0.0, N, STEPS, lv.SEED, True)


def refused_price():
    with pytest.raises(AccelerationError, match="bad payoff"):
        _hip.lvq_price(lv.S, lv.K, lv.T, lv.R, lv.Q, True, lv.TABLES["33x128"].args, 9, 0.0, N, *cc.tables(STEPS, cc.SEED_A))
    return 0


baseline = baseline_fixture(DEVICE, lambda: calls("33x128"))


HISTORIES = {
    "larger-then-smaller-table": lambda entry: [calls("64x256")[entry], calls("1x2")[entry]],
    "heston-qmc-bridge-then-n64-seedB": lambda entry: [{e.name: e for e in cc.catalogue()}["qmc-heston-bridge-n13-seedA-N257"].call,
                                                        calls("33x128", 64, cc.SEED_B)[entry]],
    "philox-price": lambda entry: [philox_price],
    "refused-price": lambda entry: [refused_price],
}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_gives_the_fresh_library_s_bits_after(baseline, entry, history):
    check_fresh_bits_after(DEVICE, baseline, entry, calls("33x128")[entry], history, HISTORIES[history](entry))
