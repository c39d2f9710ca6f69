"""tests/call_catalogue.py covers the ABI: every function include/olmc.h declares is either called by a catalogue entry or listed, with
a reason, among the exemptions the issue allows.  A new entry point fails here until it joins the catalogue.  No device, no library."""
import collections
import os
import re

from tests import call_catalogue as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOWED_EXEMPTIONS = {
    "olmc_abi_version", "olmc_init", "olmc_shutdown", "olmc_last_error", "olmc_device_info",
    "olmc_contract_layout", "olmc_multi_capacity", "olmc_heston_scenario_layout",
    "olmc_combine_cv", "olmc_combine_stats", "olmc_multi_gpu_spans",
    "olmc_tune", "olmc_profile_enable", "olmc_profile_reset", "olmc_kernel_time",
    "olmc_philox_words", "olmc_normals",             # either catalogued or exempt
}


def declared(header_text):
    """The functions the header declares: `int olmc_*(` and the one `const char* olmc_*(`."""
    return set(re.findall(r"^(?:int|const\s+char\s*\*)\s+(olmc_\w+)\s*\(", header_text, flags=re.M))


def header():
    with open(os.path.join(ROOT, "include", "olmc.h")) as f:
        return f.read()


def uncovered(header_text, entries, exempt):
    """(declared but neither catalogued nor exempt, catalogued or exempt but not declared)."""
    have = declared(header_text)
    called = {ep for e in entries for ep in e.entry_points}
    return sorted(have - called - set(exempt)), sorted((called | set(exempt)) - have)


def test_the_catalogue_and_the_exemptions_are_exactly_the_header():
    entries = cc.catalogue()
    have = declared(header())
    assert len(have) >= 79 and "olmc_european" in have and "olmc_last_error" in have
    missing, unknown = uncovered(header(), entries, cc.EXEMPT)
    assert missing == [], f"entry points without a catalogue entry: {missing}"
    assert unknown == [], f"catalogued or exempt names the header does not declare: {unknown}"
    called = {ep for e in entries for ep in e.entry_points}
    assert called.isdisjoint(cc.EXEMPT), sorted(called & set(cc.EXEMPT))
    assert set(cc.EXEMPT) <= ALLOWED_EXEMPTIONS, sorted(set(cc.EXEMPT) - ALLOWED_EXEMPTIONS)
    assert all(isinstance(reason, str) and reason.strip() for reason in cc.EXEMPT.values())
    # and the binding knows every one of them (the callables go through optionslab_amd._hip)
    assert called <= set(cc._hip.PROTOTYPES)


def test_a_new_entry_point_or_a_dropped_entry_is_noticed():
    entries = cc.catalogue()
    missing, _ = uncovered(header() + "\nint olmc_new_thing(double x, olmc_stats* out);\n", entries, cc.EXEMPT)
    assert missing == ["olmc_new_thing"]
    only = [e for e in entries if e.entry_points == ("olmc_cliquet_qmc",)]
    assert len(only) == 1
    missing, _ = uncovered(header(), [e for e in entries if e is not only[0]], cc.EXEMPT)
    assert missing == ["olmc_cliquet_qmc"]


def test_names_tags_and_callables():
    entries = cc.catalogue()
    assert 70 <= len(entries) <= 120
    names = [e.name for e in entries]
    assert len(set(names)) == len(names), [n for n, c in collections.Counter(names).items() if c > 1]
    uses = collections.Counter(tag for e in entries for tag in e.state)
    assert set(uses) == set(cc.STATE_TAGS)
    assert all(uses[tag] >= 2 for tag in cc.STATE_TAGS), uses
    for e in entries:
        assert callable(e.call) and e.state and e.entry_points, e.name
        assert set(e.sizes) == {"N", "n", "d", "k"} and all(isinstance(v, int) and v >= 0 for v in e.sizes.values()), e.name
        assert ("sobol" in e.state) == (e.sizes["d"] > 0), e.name
        assert not ({"bridge", "slabs"} & e.state) or "sobol" in e.state, e.name
        assert "slabs" not in e.state or "bridge" in e.state, e.name


def test_the_shapes_the_histories_need_are_there():
    entries = cc.catalogue()
    sobol = [e for e in entries if "sobol" in e.state]
    seeds_of_d, ds_of_seed = collections.defaultdict(set), collections.defaultdict(set)
    for e in sobol:
        seed = "seedA" if "seedA" in e.name else "seedB"
        assert seed in e.name, e.name
        seeds_of_d[e.sizes["d"]].add(seed)
        ds_of_seed[seed].add(e.sizes["d"])
    assert {5, 13, 26, 64, 128} <= set(seeds_of_d)
    assert sum(len(s) == 2 for s in seeds_of_d.values()) >= 2 and all(len(ds) >= 2 for ds in ds_of_seed.values())
    european_d = {e.sizes["d"] for e in sobol if e.entry_points == ("olmc_european_qmc",) and "seedA" in e.name}
    heston_d = {e.sizes["d"] for e in sobol if "slabs" in e.state and "seedA" in e.name}
    assert european_d & heston_d                                    # one table, two families
    for tag in ("bridge", "slabs"):
        assert {13, 64, 252} <= {e.sizes["n"] for e in entries if tag in e.state}, tag
    assert {100, 257, 4133, 70_001} <= {e.sizes["N"] for e in entries}
    assert {5, 13, 64} <= {e.sizes["n"] for e in entries}
    assert sorted(e.sizes["k"] for e in entries if "multi" in e.state) == [3, 3, 70]


def test_words_keep_every_bit():
    import numpy as np
    st = cc._hip.Stats(-0.0, float("nan"), 7, 1.5, 0.0)
    w = cc.words(st)
    assert w.dtype == np.uint64 and w.shape == (5,) and w[0] == 1 << 63 and w[2] == 7
    assert cc.words(([1.0, 2.0], [st])).shape == (7,)
    assert cc.words(np.zeros(3, dtype=np.float32)).shape == (2,)
    nan2 = np.frombuffer(np.array([0x7FF8000000000001], dtype=np.uint64).tobytes(), dtype=np.float64)
    assert not np.array_equal(cc.words(nan2), cc.words(np.array([np.nan])))
