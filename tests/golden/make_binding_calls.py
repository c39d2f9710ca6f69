#!/usr/bin/env python3
"""Generate tests/golden/binding_calls.json and tests/golden/python_refusals.json from tests/binding_calls.py.

    python tests/golden/make_binding_calls.py [output directory] [--full]

Run it on the commit BEFORE the binding's marshalling and the models' payoff plumbing were shared (or on any later one: the point of the
fixtures is that the answer is the same).  It needs neither a device nor a built library: the calls go to a recording stand-in.  The
first file holds, per driver, the symbols of the C calls it made and a digest of its whole record (every call's scalars as the argtypes
convert them, in-pointers as digests of the bytes they point to, out-pointers as null or not, and the type, shape and dtype of what the
driver returned); the second the exception type and message of every refusal of the Python layer, one fault and two faults at a time,
each message written once.  --full also writes the records themselves (binding_calls_full.json, python_refusals_full.json; not for the
repository): run it on both commits and compare those when a digest differs.  The fixtures hold names, numbers and digests only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import binding_calls as bc

    args = [a for a in sys.argv[1:] if a != "--full"]
    out = args[0] if args else HERE
    os.makedirs(out, exist_ok=True)
    calls, refusals = bc.calls(), bc.refusals()
    for name, doc, keys in (("binding_calls.json", bc.packed_calls(calls), ()), ("python_refusals.json", bc.packed_refusals(refusals), ("messages", "cases"))):
        with open(os.path.join(out, name), "w") as f:
            bc.dump_lines(doc, f, keys)
    if "--full" in sys.argv:
        for name, doc in (("binding_calls_full.json", calls), ("python_refusals_full.json", refusals)):
            with open(os.path.join(out, name), "w") as f:
                json.dump(doc, f, indent=0, sort_keys=True)
    print(len(calls), "drivers,", len(refusals), "refusals")


if __name__ == "__main__":
    main()
