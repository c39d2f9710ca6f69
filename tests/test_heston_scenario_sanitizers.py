"""The Heston scenario-set arithmetic of optionslab_amd/csrc/olmc_host_math.h (the grouping into recursions, the kernel's argument, the
Greeks' scenarios) compiled on its own by g++ with AddressSanitizer + UBSan, in the manner of tests/test_host_math_sanitizers.py: this
code needs no GPU and is not loaded into Python here.  tests/heston_scenario_harness.cpp is the driver."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("heston_scenarios") / "heston_scenario_san"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "optionslab_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "heston_scenario_harness.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed: " + build.stderr.splitlines()[0])
    assert build.returncode == 0, build.stderr

    def run(*args, stdin=""):
        r = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True,
                           env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
        assert r.returncode == 0, r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    return run


def test_property_sweep_is_clean_under_asan_and_ubsan(harness):
    """4,000 random scenario lists (1 .. 16 scenarios from pools of 1 .. 9 recursions, NaN strikes among them): the grouping against a
    brute-force one, more than six recursions refused, the kernel's slots a permutation sorted by recursion that carries each scenario's
    own constants, a recursion's first slot forming its own spot; the Greeks' scenarios for 7 / 8 / 11 / 14 contracts."""
    out = harness("self")
    assert out.startswith("ok ") and int(out.split()[1]) > 100_000


def test_grouping_in_the_header_is_the_grouping_the_library_reports(harness):
    """olmc_heston_scenario_layout of the built libolmc.so (a pure host entry point: no device) == the header compiled by g++."""
    from optionslab_amd import AccelerationError, _hip

    usual = (2.0, 0.04, 0.3, -0.7)
    scenarios = [(100.0 + i, 100.0, (1.0, 0.5, 0.1 + 0.2, 0.3)[i % 4], 0.05, 0.01 * (i % 2), i % 2 == 0, *usual, (0.04, 0.2**2, -0.01)[i % 3]) for i in range(13)]
    for sc in (scenarios, scenarios[:5], scenarios[::-1][:9]):
        lines = "\n".join(" ".join(repr(float(x)) for x in (*s[:5], *s[6:])) + f" {int(s[5])}" for s in sc)
        out = harness("layout", len(sc), stdin=lines).split()
        try:
            n_rec, group = _hip.heston_scenario_layout(sc)
        except AccelerationError:
            assert out == ["refused"]
            continue
        assert [int(x) for x in out] == [n_rec, *group]
