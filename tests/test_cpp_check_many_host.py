"""FileReference::verify_many / resilver_many's host loops (include/chunky_ec.hpp: the windows,
the report skeleton, the prepass over chunks with several locations, the CEC_PRESENT_VERIFIED
flags, the write-backs) on the CPU: tests/cpp/check_many_host_fuzz.cpp links the header against
stand-ins for cec_parts_verify and cec_parts_read that keep the C-ABI's contract and compute with
the oracle.  Random files, shapes and location mixes: verify_many gives what verify() gives file
by file; resilver_many gives the reports, location lists and final store of resilver() file by
file; what it did not write keeps its bytes; afterwards every part that had d valid chunks is
ideal; and the stand-ins see no breach of the contract (a NULL slot, a zero length, a trusted flag
on bytes that do not hash to the digest, a copy hashed twice, a part submitted twice).  Once plain,
once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program: host code only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "check_many_host_fuzz.cpp")


def _build(tmp, name, flags):
    if not (shutil.which("gcc") and shutil.which("g++")):
        pytest.skip("no host compiler")
    obj, exe = str(tmp / (name + "_oracle.o")), str(tmp / name)
    subprocess.run(["gcc", *flags, "-c", os.path.join(ROOT, "oracle", "cec_oracle.c"), "-o", obj],
                   check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I",
                    os.path.join(ROOT, "include"), SRC, obj, "-lpthread", "-o", exe], check=True)
    return exe


def _run(exe, first, count, env=None):
    r = subprocess.run([exe, str(first), str(count)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert f"{count} seeds, 0 failed, 0 contract violations" in r.stdout
    # the location mixes must reach every branch, or the fuzz passes without running it: parts
    # with a chunk of several locations (the prepass), rebuilt chunks (the write-backs), parts
    # short of d valid chunks (write_error), locations shared between chunks
    counts = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout))
    for what in ("multi_location", "rebuilt", "write_error", "shared_locations"):
        assert counts[what] > 0, r.stdout


def test_check_many_host_loop_fuzz(tmp_path):
    _run(_build(tmp_path, "check_many_host_fuzz", ["-O1"]), 0, 400)


def test_check_many_host_loop_fuzz_under_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O0"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _run(_build(tmp_path, "check_many_host_fuzz_san", san), 9000, 100, env)
