"""What the GPU test files share: the Heston pricer without its Feller warning, the tie of a launch's sums to the oracle's payoffs,
and the autouse module fixture that asserts the device and shuts the library down after the module.  Importing this needs no device.
"""
import warnings

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip


def heston_pricer(model):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                               # Feller
        return ol.HestonPricer(*model)


def check_sums(st, x, label, tie):
    """st.n, st.sum and st.sumsq against the payoffs x, within the calling file's tolerance `tie` (pytest.approx's keywords)."""
    want, want2 = float(np.sum(x)), float(np.sum(x * x))
    print(label, "sum", st.sum, "oracle", want, "sumsq", st.sumsq, "oracle", want2)
    assert st.n == len(x), label
    assert st.sum == pytest.approx(want, **tie), label
    assert st.sumsq == pytest.approx(want2, **tie), label


def device_fixture(hip=_hip, after=None):
    """The module's autouse `_device` fixture: the device is a gfx950; after the module `after` runs (knobs back at their defaults), then
    the library of `hip` (the product's binding, or the instrumented build's) shuts down."""
    @pytest.fixture(scope="module", autouse=True)
    def _device():
        info = hip.device_info()
        assert info["arch"].startswith("gfx950"), info
        yield
        if after:
            after()
        hip.shutdown()

    return _device
