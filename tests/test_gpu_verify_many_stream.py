"""FileReference::verify_many_stream (include/chunky_ec.hpp: a scrub through the scrub pipeline,
copies as segments) against verify_many, report for report, through
tests/cpp/verify_many_stream_test (built by `make -C chunky-bits_amd/csrc`): small stores with
damaged, wrong-size and missing copies and chunks with two locations, at RS(3,2) and RS(10,4),
under several segment, slot, depth and max_open settings.  One process per case, so a crash names
its case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "verify_many_stream_test")
CASES = ["stream_rs32", "stream_rs104", "refusals"]

pytestmark = pytest.mark.gpu


def test_verify_many_stream_binary_lists_its_cases():
    assert os.path.exists(BIN), "build first: make -C chunky-bits_amd/csrc"
    out = subprocess.run([BIN, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert out.stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_verify_many_stream_equals_verify_many(case):
    out = subprocess.run([BIN, case], capture_output=True, text=True, timeout=100)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{case} ... ok" in out.stdout
