"""FileReference::read_many's host loop (include/chunky_ec.hpp: the gathering of parts per shape,
the draw of d chunks per part, the retry rounds with CEC_PRESENT_VERIFIED flags) on the CPU:
tests/cpp/read_many_host_fuzz.cpp links the header against a stand-in cec_parts_read that keeps
the C-ABI's contract and computes with the oracle.  Random files, shapes and location mixes:
read_many gives the files' bytes and what read() gives file by file, a part without d good chunks
fails it with TooFewShardsPresent as it fails read(), and the stand-in sees no breach of the
contract (a NULL slot it must read or fill, a trusted flag on a chunk it never verified, a
finished part submitted again).  Once plain, once under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program: host code only)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "read_many_host_fuzz.cpp")


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
    # the location mixes must make some parts go up again, or the retry rounds are not run
    retried = int(r.stdout.split("(")[1].split()[0])
    assert retried > 0, r.stdout


def test_read_many_host_loop_fuzz(tmp_path):
    _run(_build(tmp_path, "read_many_host_fuzz", ["-O1"]), 0, 400)


def test_read_many_host_loop_fuzz_under_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O0"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _run(_build(tmp_path, "read_many_host_fuzz_san", san), 7000, 100, env)
