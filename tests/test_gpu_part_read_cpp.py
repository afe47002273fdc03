"""FilePart::read_coalesced (include/chunky_ec.hpp) against read_with_context with 16 concurrent
readers of parts of different sizes, through tests/cpp/part_read_test (built by
`make -C chunky-bits_amd/csrc`): one process per case, so a crash names its case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "part_read_test")
CASES = ["rs32", "rs104", "too_few"]

pytestmark = pytest.mark.gpu


def test_part_read_binary_lists_its_cases():
    assert os.path.exists(BIN), "build first: make -C chunky-bits_amd/csrc"
    out = subprocess.run([BIN, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert out.stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_read_coalesced_equals_read_with_context(case):
    out = subprocess.run([BIN, case], capture_output=True, text=True, timeout=100)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{case} ... ok" in out.stdout
