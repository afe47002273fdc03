"""The batch planning of write_many_stream under many_segment
(include/chunky_ec_segment_plan.hpp): which segments form the next batch, the slot budget, the
allocation of open ids and the hold-back order.  Pure host code; tests/cpp/segment_plan_test.cpp
checks it on the CPU over seeded random part lists, also against the segment pipeline's own rule
table (csrc/segment_words.hpp), plain and under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chunky-bits_amd", "csrc")
INC = os.path.join(ROOT, "include")


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_segment_plan_rules_hold_over_random_part_lists():
    """The program the library's build leaves beside its source."""
    exe = os.path.join(ROOT, "tests", "cpp", "segment_plan_test")
    assert os.path.exists(exe), "build() makes tests/cpp/segment_plan_test"
    r = _run([exe])
    assert r.returncode == 0 and "segment_plan ok: 162 random part lists" in r.stdout, r.stdout


def test_segment_plan_rules_under_sanitizers(tmp_path):
    """The same program (host code only, its own main) built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "segment_plan_san")
    r = _run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", INC,
              os.path.join(ROOT, "tests", "cpp", "segment_plan_test.cpp"), "-o", exe])
    assert r.returncode == 0, r.stdout
    r = _run([exe])
    assert r.returncode == 0 and "segment_plan ok" in r.stdout, r.stdout
