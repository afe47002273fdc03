"""The per-call tier's layout rules (csrc/percall_plan.hpp): where a batch of gathered
cec_part_encode calls lies (one chunk length: the strided block; two or more: the split layout)
and which byte ranges a host-staged read moves up and brings back.  The rules are pure functions
the host compiles without the HIP runtime; tests/cpp/percall_plan_test.cpp checks them on the CPU
over seeded random batches, plain and under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chunky-bits_amd", "csrc")


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_percall_plan_rules_hold_over_random_batches():
    """The program the library's build leaves beside its source."""
    exe = os.path.join(ROOT, "tests", "cpp", "percall_plan_test")
    assert os.path.exists(exe), "build() makes tests/cpp/percall_plan_test"
    r = _run([exe])
    assert r.returncode == 0 and "percall_plan ok: 160 random batches" in r.stdout, r.stdout


def test_percall_plan_rules_under_sanitizers(tmp_path):
    """The same program (host code only, its own main) built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "percall_plan_san")
    r = _run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=undefined", "-I", CSRC,
              os.path.join(ROOT, "tests", "cpp", "percall_plan_test.cpp"), "-o", exe])
    assert r.returncode == 0, r.stdout
    r = _run([exe])
    assert r.returncode == 0 and "percall_plan ok" in r.stdout, r.stdout
