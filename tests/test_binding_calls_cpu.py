"""The Python layer makes the C calls, and the refusals, it made before its marshalling was shared: tests/binding_calls.py's drivers are
replayed against a recording stand-in for the library and compared, driver by driver, with tests/golden/binding_calls.json (the symbols
reached and a digest of the whole record: equal digests are equal records) and, refusal by refusal, with
tests/golden/python_refusals.json (tests/golden/make_binding_calls.py, run on the parent commit; its --full writes the records behind a
digest).  Neither a device nor libolmc.so is needed."""
import json
import os
import subprocess
import sys

import pytest

from tests import binding_calls as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def golden_calls():
    """{label: "symbols digest"}, the fixture's groups merged."""
    return {label: packed for group in golden("binding_calls.json").values() for label, packed in group.items()}


def golden_refusals():
    """{label: [type, message] or "none"}."""
    doc = golden("python_refusals.json")
    return {f"{case}/{faults}": ("none" if i < 0 else doc["messages"][i]) for case, group in doc["cases"].items() for faults, i in group.items()}


@pytest.fixture(scope="module")
def replayed():
    return bc.calls()


def test_the_drivers_are_the_recorded_ones_and_cover_what_the_issue_lists(replayed):
    want = golden_calls()
    assert sorted(replayed) == sorted(want)
    from tests import call_catalogue as cc

    skipped = [e.name for e in cc.catalogue() if f"catalogue/{e.name}" not in want]
    assert len(skipped) == 3 and all("caller_stream" in e.state for e in cc.catalogue() if e.name in skipped)
    symbols = {label: packed.split(" ")[0].split("+") for label, packed in want.items()}
    reached = {symbol for called in symbols.values() for symbol in called}
    never = set(bc.prototypes()) - reached
    assert never <= set(cc.EXEMPT) | {"olmc_european_shard_dev"}, sorted(never)        # every compute entry point but the caller-stream one is recorded
    assert {"olmc_fetch_dev", "olmc_contract_layout", "olmc_heston_scenario_layout", "oljd_autocallable", "oljd_cliquet"} <= reached
    assert all(len(symbols[f"method/{m}-price_surface{tail}"]) == 2                # 18 cells: two launches each
               for m, tail in (("heston-pseudo-bridge-euler", ""), ("heston-qmc-sequential-qe", ""), ("dupire", ""), ("dupire-qmc-bridge", ""),
                               ("merton", "-anti0"), ("kou", "-anti1")))


def test_every_driver_makes_the_recorded_c_calls_and_returns_the_recorded_shape(replayed):
    want = golden_calls()
    now = {label: packed for group in bc.packed_calls(replayed).values() for label, packed in group.items()}
    wrong = [label for label in want if now.get(label) != want[label]]
    for label in wrong[:3]:
        print(label, "\n  recorded", want[label], "\n  now     ", now.get(label), "\n  now, in full", replayed.get(label))
    assert not wrong, wrong


def test_every_refusal_keeps_its_type_message_and_order():
    want, got = golden_refusals(), bc.refusals()
    assert sorted(got) == sorted(want)
    wrong = {label: (want[label], got[label]) for label in want if got[label] != want[label]}
    assert not wrong, wrong
    assert all(v == "none" or len(v) == 2 for v in got.values())        # no refusal came after the library was asked for or called
    assert sum(1 for v in want.values() if v != "none") > 500 and sum(1 for label in want if "+" in label) > 300


def test_the_refusals_come_before_the_library_is_loaded():
    code = ("from tests import binding_calls as bc\n"
            "from optionslab_amd import _hip\n"
            "doc = bc.refusals()\n"
            "assert doc and all(v == 'none' or len(v) == 2 for v in doc.values()), [k for k, v in doc.items() if len(v) == 3]\n"
            "assert _hip._lib is None, 'the library was loaded'\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
