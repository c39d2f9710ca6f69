"""The oljd_* entry points give the bits of a freshly initialised library whatever ran before them.

tests/test_gpu_local_vol_qmc_history.py's bar for include/olmc_jump.h: the BASELINE of a call is the same call as the first one after
olmc_shutdown, results are compared as uint64 words (call_catalogue.words), and once a call fails unexpectedly nothing more is started
on the device.  Each of the five entry points (257 x 13, Merton M0) runs after
  (a) the same entry point with Kou K1 at n = 64 and another seed (longer walks, other size blocks, a larger matrix);
  (b) the catalogue's olmc_heston_qmc bridge call at 13 steps (tables, plan and slabs on the same context);
  (c) olmc_jump_diffusion (the kernel whose stream these share);
  (d) a refused oljd_price (an argument error, made before any device work).
"""
import pytest

from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import call_catalogue as cc
from tests import heston_path_oracle as hpo
from tests.history import Device, baseline_fixture, check_fresh_bits_after

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

S, K, T, R, Q, SIGMA = hpo.S, hpo.K, hpo.T, hpo.R, hpo.Q, 0.2
N, STEPS = 257, 13
M0, K1 = (False, 0.5, -0.1, 0.2, 0.0), (True, 60.0, 0.6, 25.0, 20.0)
AUTOCALL, CLIQUET = (1.0, 0.9, 0.10, 0.8), (0.05, -0.05, 0.30, 0.0)
ENTRIES = ["oljd_price", "oljd_surface_prices", "oljd_autocallable", "oljd_cliquet", "oljd_paths"]
DEVICE = Device()


def calls(model=M0, n=STEPS, seed=cc.SEED_A):
    return {
        "oljd_price": lambda: [_hip.jd_price(S, K, T, R, SIGMA, Q, True, model, code, level, N, n, seed, True)
                               for code, level in ((0, hpo.UP), (3, hpo.DOWN), (5, 0.0), (6, 0.0), (7, 0.0), (_hip.JD_EUROPEAN, 0.0))],
        "oljd_surface_prices": lambda: _hip.jd_surface_prices(S, T, R, SIGMA, Q, False, model, [95.0, 105.0, 100.0], [n, 4, 5], N, n, seed, True),
        "oljd_autocallable": lambda: _hip.jd_autocallable(S, T, R, SIGMA, Q, model, *AUTOCALL, 4, N, n, seed, True),
        "oljd_cliquet": lambda: _hip.jd_cliquet(S, T, R, SIGMA, Q, model, *CLIQUET, 4, N, n, seed, False),
        "oljd_paths": lambda: [_hip.jd_paths(S, T, R, SIGMA, Q, model, N, n, seed, mirror=m, path_major=True) for m in (False, True)],
    }


def old_price():
    return _hip.jump_diffusion(S, K, T, R, SIGMA, Q, True, *K1, 4133, 64, cc.SEED_B)


def refused_price():
    with pytest.raises(AccelerationError, match="bad payoff"):
        _hip.jd_price(S, K, T, R, SIGMA, Q, True, M0, 9, 0.0, N, STEPS, cc.SEED_A)
    return 0


baseline = baseline_fixture(DEVICE, lambda: calls())


HISTORIES = {
    "k1-n64-seedB": lambda entry: [calls(K1, 64, cc.SEED_B)[entry]],
    "heston-qmc-bridge": lambda entry: [{e.name: e for e in cc.catalogue()}["qmc-heston-bridge-n13-seedA-N257"].call],
    "olmc-jump-diffusion": lambda entry: [old_price],
    "refused-price": lambda entry: [refused_price],
}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_gives_the_fresh_library_s_bits_after(baseline, entry, history):
    check_fresh_bits_after(DEVICE, baseline, entry, calls()[entry], history, HISTORIES[history](entry))
