"""What the fresh-library tests share: the latch that stops a file's device work, the word-by-word report, the family test's body.

A history test compares a call's result, as uint64 words (call_catalogue.words), with the same call as the first one after
olmc_shutdown.  Each test file makes its own Device: once a call of that file fails with anything but the refusal its history expects,
every later call of the file fails at once without starting anything more on the device.  tests/test_history_cpu.py checks this
module with stand-in callables, without a library.
"""
import time

import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import call_catalogue as cc


class Device:
    """The latch of one test file.  `record` turns what a call returns into what the file compares (the result's words)."""

    def __init__(self, record=cc.words):
        self.record = record
        self.dead = []            # the message of a call that failed unexpectedly: nothing more is started on the device

    def _alive(self):
        if self.dead:
            pytest.fail(f"an earlier call failed, nothing more is run on the device: {self.dead[0]}")

    def invoke(self, label, call):
        self._alive()
        try:
            return self.record(call())
        except BaseException as exc:
            self.dead.append(f"{label}: {type(exc).__name__}: {exc}")
            raise

    def fresh(self, label, call):
        """The call as the first one of a newly initialised library."""
        _hip.shutdown()
        return self.invoke(label, call)

    def guarded(self, label, call):
        """Runs an early-return call; anything but the outcome its history expects ends the device work of this file."""
        self._alive()
        try:
            return call()
        except BaseException as exc:
            if isinstance(exc, ol.AccelerationError) and "libolmc error 1:" in str(exc):      # OLMC_ERR_ARG: refused before any device work
                return exc
            self.dead.append(f"{label}: {type(exc).__name__}: {exc}")
            raise


def first_difference(got, want) -> str:
    if got.shape != want.shape:
        return f"{got.size} words instead of {want.size}"
    i = int(np.flatnonzero(got != want)[0])
    return (f"word {i} of {want.size}: got 0x{int(got[i]):016x} ({got[i:i + 1].view(np.float64)[0]!r}), "
            f"fresh library 0x{int(want[i]):016x} ({want[i:i + 1].view(np.float64)[0]!r}); {int(np.count_nonzero(got != want))} words differ")


def baseline_fixture(device, calls, defaults=None):
    """The module's `baseline` fixture: label -> words of calls()[label] on a fresh library, taken once.  `defaults` (the knobs at their
    defaults, profiling off) runs before, and again after the module unless the device is latched."""
    @pytest.fixture(scope="module")
    def baseline():
        if not _hip.hip_available():
            pytest.fail("no HIP device")
        if defaults:
            defaults()
        t0 = time.perf_counter()
        base = {label: device.fresh(label, call) for label, call in calls().items()}
        print(f"\nBASELINE {len(base)} fresh libraries in {time.perf_counter() - t0:.2f} s")
        yield base
        if defaults and not device.dead:
            defaults()

    return baseline


def check_fresh_bits_after(device, baseline, entry, call, history, before):
    """The calls of `before` on a fresh library, then `call` twice: both times the words of baseline[entry]."""
    _hip.shutdown()
    for i, earlier in enumerate(before):
        device.invoke(f"{history}, call {i + 1}, before {entry}", earlier)
    got, want = device.invoke(entry, call), baseline[entry]
    assert np.array_equal(got, want), f"{entry} after {history}: {first_difference(got, want)}"
    again = device.invoke(entry, call)                                 # and once more on the used library
    assert np.array_equal(again, want), f"{entry} after {history}, on the used library: {first_difference(again, want)}"
