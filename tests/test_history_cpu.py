"""tests/history.py and abi_support.refused with stand-in callables: no device, no library.

The latch and the refusal runner are what the GPU history files and the refusal tables rest on; a latch that lets a call through after a
failure, or a runner that skips the message, would leave all of those passing.  Here both are made to fail.
"""
import numpy as np
import pytest

import optionslab_amd as ol
from optionslab_amd import _hip
from tests import history
from tests.abi_support import no_library, refused  # noqa: F401  (no_library is a fixture)


class Counted:
    """A call that counts itself and returns `value`, or raises it if it is an exception."""

    def __init__(self, value=None):
        self.value, self.calls = value, 0

    def __call__(self):
        self.calls += 1
        if isinstance(self.value, BaseException):
            raise self.value
        return self.value


@pytest.fixture
def shutdowns(no_library, monkeypatch):
    """_hip.shutdown replaced by a counter, and the library out of reach."""
    counted = Counted()
    monkeypatch.setattr(_hip, "shutdown", counted)
    monkeypatch.setattr(_hip, "load_library", lambda: pytest.fail("the library was loaded"))
    return counted


def device():
    return history.Device(record=lambda result: result)


def failed(call) -> str:
    with pytest.raises(pytest.fail.Exception) as e:
        call()
    return str(e.value)


def test_invoke_returns_what_record_makes_of_the_result(shutdowns):
    d = history.Device(record=lambda result: result + 1)
    assert d.invoke("one", Counted(41)) == 42 and d.fresh("two", Counted(1)) == 2
    assert shutdowns.calls == 1 and not d.dead


def test_after_a_call_that_raised_nothing_more_is_called(shutdowns):
    d, bad, later = device(), Counted(RuntimeError("the queue is gone")), Counted(7)
    with pytest.raises(RuntimeError):
        d.invoke("first", bad)
    assert bad.calls == 1 and d.dead == ["first: RuntimeError: the queue is gone"]
    for entry in (lambda: d.invoke("second", later), lambda: d.fresh("third", later), lambda: d.guarded("fourth", later)):
        assert "first: RuntimeError: the queue is gone" in failed(entry)
    assert later.calls == 0
    with pytest.raises(ValueError):                                  # a second file's latch is its own
        device().invoke("other file", Counted(ValueError("x")))
    assert len(d.dead) == 1


def test_a_failure_inside_fresh_and_inside_record_latches_too(shutdowns):
    d = device()
    with pytest.raises(KeyboardInterrupt):
        d.fresh("interrupted", Counted(KeyboardInterrupt()))
    assert shutdowns.calls == 1 and d.dead == ["interrupted: KeyboardInterrupt: "]

    def no_words(result):
        raise TypeError("no words in " + repr(result))

    d = history.Device(record=no_words)
    with pytest.raises(TypeError):
        d.invoke("odd result", Counted(3))
    assert d.dead == ["odd result: TypeError: no words in 3"]


def test_guarded_returns_an_argument_refusal_and_latches_on_everything_else(shutdowns):
    d = device()
    refusal = ol.AccelerationError("libolmc error 1: bad payoff", backend="hip")
    assert d.guarded("refused", Counted(refusal)) is refusal and not d.dead
    assert d.guarded("fine", Counted(5)) == 5 and d.invoke("still alive", Counted(6)) == 6
    fault = ol.AccelerationError("libolmc error 3: an illegal memory access was encountered", backend="hip")
    with pytest.raises(ol.AccelerationError):
        d.guarded("faulted", Counted(fault))
    assert d.dead == [f"faulted: AccelerationError: {fault}"]
    d = device()
    with pytest.raises(ZeroDivisionError):
        d.guarded("other", Counted(ZeroDivisionError("1/0")))
    assert d.dead == ["other: ZeroDivisionError: 1/0"]
    assert shutdowns.calls == 0


def test_the_family_test_s_body_compares_both_calls_and_stops_at_the_latch(shutdowns):
    want = np.arange(4, dtype=np.uint64)
    d, before, call = device(), Counted(want), Counted(want.copy())
    history.check_fresh_bits_after(d, {"entry": want}, "entry", call, "some history", [before, before])
    assert (shutdowns.calls, before.calls, call.calls) == (1, 2, 2)
    other = want.copy()
    other[2] = 9
    with pytest.raises(AssertionError, match="entry after some history: word 2 of 4: got 0x0000000000000009"):
        history.check_fresh_bits_after(d, {"entry": want}, "entry", Counted(other), "some history", [])
    assert not d.dead                                                # a difference is a failed test, not a failed call
    with pytest.raises(OSError):
        history.check_fresh_bits_after(d, {"entry": want}, "entry", call, "a history that fails", [Counted(OSError("gone"))])
    assert call.calls == 2 and d.dead == ["a history that fails, call 1, before entry: OSError: gone"]


def test_first_difference_reports_sizes_and_the_first_differing_word():
    want = np.array([1.0, np.nan, -0.0, 2.5]).view(np.uint64)
    assert history.first_difference(want[:3], want) == "3 words instead of 4"
    got = want.copy()
    got[1] ^= np.uint64(1)                                           # another NaN payload: equal as floats to nothing, different as words
    got[3] = np.array([2.75]).view(np.uint64)[0]
    assert np.isnan(got.view(np.float64)[1]) and not np.array_equal(got, want)
    text = history.first_difference(got, want)
    assert text.startswith("word 1 of 4: got 0x7ff8000000000001 (") and "fresh library 0x7ff8000000000000 (" in text and text.endswith("; 2 words differ")
    got = want.copy()
    got[2] = 0                                                       # +0.0 for -0.0
    text = history.first_difference(got, want)
    assert text.startswith("word 2 of 4: got 0x0000000000000000 (") and "fresh library 0x8000000000000000 (" in text and text.endswith("; 1 words differ")


class StandInLibrary:
    def __init__(self, message):
        self.message = message

    def olmc_last_error(self):
        return self.message.encode()


def test_refused_fails_on_a_wrong_return_code_and_on_a_wrong_message():
    lib = StandInLibrary("n_paths must be >= 1")
    refused(lib, 1, "n_paths must be >= 1")
    for rc in (0, 2, -1):
        with pytest.raises(AssertionError):
            refused(lib, rc, "n_paths must be >= 1")
    with pytest.raises(AssertionError):
        refused(lib, 1, "n_steps must be >= 1")
    with pytest.raises(AssertionError):
        refused(lib, 1, "n_paths must be >= 1 ")
