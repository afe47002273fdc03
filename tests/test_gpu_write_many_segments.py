"""FileWriteBuilder::write_many_stream under many_segment (include/chunky_ec.hpp: gathered parts
streamed through the segment pipeline, long chunks as column segments) against write() file by
file, through tests/cpp/write_many_segments_test (built by `make -C chunky-bits_amd/csrc`): one
process per case, so a crash names its case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "write_many_segments_test")
CASES = ["long_and_short_interleaved", "exact_multiples_of_the_segment", "empty_files",
         "full_parts_in_the_middle", "max_open_reached", "option_rules"]

pytestmark = pytest.mark.gpu


def test_write_many_segments_binary_lists_its_cases():
    assert os.path.exists(BIN), "build first: make -C chunky-bits_amd/csrc"
    out = subprocess.run([BIN, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert out.stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_write_many_stream_with_segments_equals_write(case):
    out = subprocess.run([BIN, case], capture_output=True, text=True, timeout=100)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{case} ... ok" in out.stdout
