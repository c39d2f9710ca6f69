"""The olsq_* entry points give the bits of a freshly initialised library whatever ran before them.

tests/test_gpu_sabr_history.py's bar for include/olmc_sabr_qmc.h: the BASELINE of a call is the same call as the first one after
olmc_shutdown, results are compared as uint64 words (call_catalogue.words), and once a call fails unexpectedly nothing more is started
on the device.  What a context keeps for this family: the Sobol tables and the bridge plan of the last call, and the bridge slabs it
shares with the Heston and local-volatility Sobol kernels.  Each of the three entry points (bridge, 257 x 13 on `half`) runs after
  (a) the same entry point on the general and the absorbing beta = 0 kernels, and sequentially at n = 64;
  (b) the catalogue's olmc_heston_qmc bridge call at 13 steps, then its bridge call at 252 steps, which leaves a larger slab behind on
      the same context;
  (c) an olvq_price bridge call, which uses the same slab block at [n][64];
  (d) olsb_price on the same model (the Philox kernels: the model in units of the raw normals);
  (e) a refused olsq_price (an argument error, made before any device work).
"""
import pytest

from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import call_catalogue as cc
from tests import sabr_oracle as so
from tests import test_gpu_local_vol as lv
from tests.history import Device, baseline_fixture, check_fresh_bits_after

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

N, STEPS = 257, 13
K = 100.0
ENTRIES = ["olsq_price", "olsq_paths", "olsq_surface_prices"]
DEVICE = Device()


def cells(n):
    return [95.0, 105.0, 100.0], [n, 4, 5]


def calls(name, n=STEPS, bridge=True):
    """The three entry points on model `name` of tests/sabr_oracle.py."""
    model = so.MODELS[name]
    tables = lambda: cc.tables(2 * n, cc.SEED_A)
    return {
        "olsq_price": lambda: [_hip.sabrq_price(so.F0, K, so.T, so.R, True, model, code, level, N, *tables(), bridge, True)
                               for code, level in ((0, so.UP), (3, so.DOWN), (6, 0.0), (7, 0.0), (_hip.SABR_EUROPEAN, 0.0))],
        "olsq_paths": lambda: list(_hip.sabrq_paths(so.F0, so.T, model, N, *tables(), bridge, mirror=True, path_major=True)),
        "olsq_surface_prices": lambda: _hip.sabrq_surface_prices(so.F0, so.T, so.R, False, model, *cells(n), N, *tables(), bridge, True),
    }


def catalogue_call(name):
    return {e.name: e for e in cc.catalogue()}[name].call


def local_vol_bridge_price():
    return _hip.lvq_price(lv.S, lv.K, lv.T, lv.R, lv.Q, True, lv.TABLES["33x128"].args, 6, 0.0, N, *cc.tables(STEPS, cc.SEED_A), True, True)


def philox_price():
    return _hip.sabr_price(so.F0, K, so.T, so.R, True, so.MODELS["half"], 6, 0.0, N, STEPS, so.SEED, True)


def refused_price():
    with pytest.raises(AccelerationError, match="bad payoff"):
        _hip.sabrq_price(so.F0, K, so.T, so.R, True, so.MODELS["half"], 9, 0.0, N, *cc.tables(2 * STEPS, cc.SEED_A))
    return 0


baseline = baseline_fixture(DEVICE, lambda: calls("half"))


HISTORIES = {
    "other-beta-kinds-then-sequential-n64": lambda entry: [calls("general")[entry], calls("normal-absorbing")[entry], calls("half", 64, False)[entry]],
    "heston-qmc-bridge-n13-then-n252": lambda entry: [catalogue_call("qmc-heston-bridge-n13-seedA-N257"), catalogue_call("qmc-heston-bridge-n252-seedA-N100")],
    "local-vol-qmc-bridge-price": lambda entry: [local_vol_bridge_price],
    "philox-price": lambda entry: [philox_price],
    "refused-price": lambda entry: [refused_price],
}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_gives_the_fresh_library_s_bits_after(baseline, entry, history):
    check_fresh_bits_after(DEVICE, baseline, entry, calls("half")[entry], history, HISTORIES[history](entry))
