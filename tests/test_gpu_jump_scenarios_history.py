"""The oljs_* compute entry points give the bits of a freshly initialised library whatever ran before them.

tests/test_gpu_jump_history.py's bar for include/olmc_jump_scenarios.h: the BASELINE of a call is the same call as the first one after
olmc_shutdown, results are compared as uint64 words (call_catalogue.words), and once a call fails unexpectedly nothing more is started
on the device.  Each of the two entry points (257 x 13, Merton and a mixed set of seven groups) runs after
  (a) the same entry point with Kou at n = 64 and another seed (longer walks, many size blocks, another group bound);
  (b) the catalogue's olmc_heston_qmc bridge call at 13 steps (tables, plan and slabs on the same context);
  (c) oljd_price (the one-contract kernels whose stream these share);
  (d) a refused oljs_scenarios (an argument error, made before any device work).
"""
import pytest

from optionslab_amd import _hip
from optionslab_amd.exceptions import AccelerationError
from tests import call_catalogue as cc
from tests import jump_scenario_cases as jc
from tests.history import Device, baseline_fixture, check_fresh_bits_after

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The balance properties of Sobol")]

S, K, T, R, Q, SIGMA = jc.S, jc.K, jc.T, jc.R, jc.Q, jc.SIGMA
N, STEPS = 257, 13
ENTRIES = ["oljs_scenarios", "oljs_greeks_fd"]
DEVICE = Device()


def calls(model=jc.MERTON, n=STEPS, seed=cc.SEED_A):
    return {
        "oljs_scenarios": lambda: [_hip.jd_scenarios(jc.mixed_set(model), N, n, seed, True), _hip.jd_scenarios(jc.greeks_set(model)[:3], N, n, seed, False)],
        "oljs_greeks_fd": lambda: [list(part) for second in (True, False)
                                   for part in _hip.jd_greeks_fd(S, K, T, R, SIGMA, Q, second, model, N, n, seed, second, second)],
    }


def one_contract():
    return _hip.jd_price(S, K, T, R, SIGMA, Q, True, jc.KOU, 6, 0.0, 4133, 64, cc.SEED_B, True)


def refused_scenarios():
    with pytest.raises(AccelerationError, match="T must be > 0 in every scenario"):
        _hip.jd_scenarios([jc.scenario(), jc.scenario(T_=0.0)], N, STEPS, cc.SEED_A)
    return 0


baseline = baseline_fixture(DEVICE, lambda: calls())


HISTORIES = {
    "kou-n64-seedB": lambda entry: [calls(jc.KOU, 64, cc.SEED_B)[entry]],
    "heston-qmc-bridge": lambda entry: [{e.name: e for e in cc.catalogue()}["qmc-heston-bridge-n13-seedA-N257"].call],
    "oljd-price": lambda entry: [one_contract],
    "refused-scenarios": lambda entry: [refused_scenarios],
}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_gives_the_fresh_library_s_bits_after(baseline, entry, history):
    check_fresh_bits_after(DEVICE, baseline, entry, calls()[entry], history, HISTORIES[history](entry))
