"""FileReference::read_many_stream (include/chunky_ec.hpp) against read_many and the written
bytes, through tests/cpp/read_many_stream_test (built by `make -C chunky-bits_amd/csrc`): one
process per case, so a crash names its case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "read_many_stream_test")
CASES = ["rs32", "rs104", "mixed_batch", "damaged_rs32", "damaged_rs104", "small_slots", "too_few",
         "refused_shape", "released"]

pytestmark = pytest.mark.gpu


def test_read_many_stream_binary_lists_its_cases():
    assert os.path.exists(BIN), "build first: make -C chunky-bits_amd/csrc"
    out = subprocess.run([BIN, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert out.stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_read_many_stream_equals_read_many(case):
    out = subprocess.run([BIN, case], capture_output=True, text=True, timeout=100)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{case} ... ok" in out.stdout
