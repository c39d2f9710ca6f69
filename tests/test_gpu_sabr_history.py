"""The SABR entry points give the bits of a freshly initialised library whatever ran before them.

tests/test_gpu_local_vol_history.py's bar for include/olmc_sabr.h: the BASELINE of a call is the same call as the first one after
olmc_shutdown (the next call initialises a new library), results are compared as uint64 words (call_catalogue.words), and once a call
fails unexpectedly nothing more is started on the device.  This family keeps nothing of its own on a context; it shares the workspace
of every reducing call and the bulk buffer of every matrix call.  Each of the three entry points, at N = 257 and n = 13 on the beta = 0.5
model, runs after
  (a) the same entry point on another kind of beta (the general kernel, then the absorbing beta = 0 one);
  (b) an olmc_heston_qmc bridge call (Sobol table, bridge plan and slabs on the same context);
  (c) a refused olsb_price (an argument error, made before any device work).
"""
import pytest

from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import call_catalogue as cc
from tests import sabr_oracle as so
from tests.history import Device, baseline_fixture, check_fresh_bits_after

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

N, STEPS = 257, 13
K = 100.0
CELLS = ([95.0, 105.0, 100.0], [13, 4, 5])
DEVICE = Device()


def calls(name):
    """The three entry points on model `name` of tests/sabr_oracle.py."""
    model = so.MODELS[name]
    return {
        "olsb_price": lambda: [_hip.sabr_price(so.F0, K, so.T, so.R, True, model, code, level, N, STEPS, so.SEED, True)
                               for code, level in ((0, so.UP), (3, so.DOWN), (6, 0.0), (7, 0.0), (_hip.SABR_EUROPEAN, 0.0))],
        "olsb_paths": lambda: list(_hip.sabr_paths(so.F0, so.T, model, N, STEPS, so.SEED, mirror=True, path_major=True)),
        "olsb_surface_prices": lambda: _hip.sabr_surface_prices(so.F0, so.T, so.R, False, model, *CELLS, N, STEPS, so.SEED, True),
    }


def refused_price():
    with pytest.raises(AccelerationError, match="bad payoff"):
        _hip.sabr_price(so.F0, K, so.T, so.R, True, so.MODELS["half"], 9, 0.0, N, STEPS, so.SEED)
    return 0


baseline = baseline_fixture(DEVICE, lambda: calls("half"))


HISTORIES = {
    "another-beta-kind": lambda entry: [calls("general")[entry], calls("normal-absorbing")[entry]],
    "heston-qmc-bridge": lambda entry: [{e.name: e for e in cc.catalogue()}["qmc-heston-bridge-n13-seedA-N257"].call],
    "refused-price": lambda entry: [refused_price],
}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("entry", ["olsb_price", "olsb_paths", "olsb_surface_prices"])
def test_entry_point_gives_the_fresh_library_s_bits_after(baseline, entry, history):
    check_fresh_bits_after(DEVICE, baseline, entry, calls("half")[entry], history, HISTORIES[history](entry))
