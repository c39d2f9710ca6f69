"""What the *_cpu.py files share on the C-ABI side: the loaded library, the arguments of refusal rows, the refusal check, the
header / exports / prototypes check, and the two fixtures that fail a test which reaches the library or the device.

Test modules import the fixtures by name (`from tests.abi_support import library`), so each module gets its own instance.  The
_REFUSALS tables stay in their files: they are the assertions, `refused` is only their runner.
"""
import ctypes as C
import re
import subprocess

import pytest

from optionslab_amd import _hip
from optionslab_amd.build import LIBRARY, build_library


@pytest.fixture(scope="module")
def library():
    build_library()
    return _hip.load_library()


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library (hence to reach the device) fails the test."""
    def touched(*a, **k):
        raise AssertionError("the library was loaded: the device would be touched")

    monkeypatch.setattr(_hip, "lib", touched)


@pytest.fixture
def no_device(request, monkeypatch):
    """Any attempt to reach the library (hence the device) through one of the test module's _BINDINGS fails the test.  Every name must
    exist in _hip: a binding that was renamed fails here, it is not patched into being."""
    def touched(*a, **k):
        raise AssertionError("the device was touched")

    for name in request.module._BINDINGS:
        monkeypatch.setattr(_hip, name, touched)


# ----------------------------------------------------------------------------------------- arguments of refusal rows ----
def _ST():
    return C.byref(_hip.Stats())


def _CV():
    return C.byref(_hip.CvMoments())


def _out(n_points, n_steps):
    return (C.c_double * (n_points * (n_steps + 1)))()


def _out9():
    return (C.c_double * 9)()


def _out17():
    return (_hip.Stats * 17)()


def _opts(k):
    return (_hip.Option * 16)(*[_hip.Option(100.0, 90.0 + i, 1.0, 0.05, 0.2, 0.0, 1, 0) for i in range(k)])


def sobol(dims):
    """Stand-in direction numbers and shifts: never read, every call that takes them here is refused first."""
    return (C.c_uint32 * (30 * max(dims, 1)))(*range(1, 30 * max(dims, 1) + 1)), (C.c_uint32 * max(dims, 1))()


# -------------------------------------------------------------------------------------------------------- the checks ----
def refused(library, rc, message):
    """The call answered OLMC_ERR_ARG (1) with its exact message."""
    assert rc == 1
    assert library.olmc_last_error().decode() == message


def assert_header_matches(library, header_path, prefix, prototypes, names):
    """The header's declarations = the library's exports = the ctypes prototypes = names, for the entry points that begin with prefix;
    every bound function carries its prototype; no name is shared with another family's table; the ABI version stays 6."""
    text = re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)
    declared = sorted(set(re.findall(rf"\b({prefix}[a-z0-9_]+)\s*\(", text)))
    out = subprocess.run(["nm", "-D", "--defined-only", LIBRARY], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(rf"\bT ({prefix}[a-z0-9_]+)", out)))
    assert declared == exported == sorted(prototypes) == sorted(names)
    for name, (res, args) in prototypes.items():
        fn = getattr(library, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    for other in (_hip.PROTOTYPES, _hip.LV_PROTOTYPES, _hip.LVQ_PROTOTYPES, _hip.JD_PROTOTYPES):
        assert other is prototypes or not set(prototypes) & set(other)
    assert library.olmc_abi_version() == 6
