"""FileReference::verify_many_stream's host loop (include/chunky_ec.hpp: the copy list under the
skeleton rule, detail::SegmentPlanner's batches with one chunk per part, the expected rows, the
verdicts' collection and the summaries) on the CPU: tests/cpp/verify_many_stream_host_fuzz.cpp
links the header against stand-ins for cec_scrub_pipeline_* that enforce the contract of
include/chunky_ec_scrub.h (the engine's own open-id table from csrc/segment_words.hpp, the slot's
capacity, an expected row read only where a copy ends, no id reused before its LAST, verdicts
readable only between wait and the next acquire) and compute with the oracle's SHA-256 over the
bytes accumulated per open id.  Random files, shapes and location mixes (good, damaged, short and
missing copies): verify_many_stream gives what verify() gives file by file, for several segment
and slot sizes, a slot of one segment and max_open = 1 among them.  Once plain, once under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program: host code only)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "verify_many_stream_host_fuzz.cpp")


def _build(tmp, name, flags):
    if not (shutil.which("gcc") and shutil.which("g++")):
        pytest.skip("no host compiler")
    obj, exe = str(tmp / (name + "_oracle.o")), str(tmp / name)
    subprocess.run(["gcc", *flags, "-c", os.path.join(ROOT, "oracle", "cec_oracle.c"), "-o", obj],
                   check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "chunky-bits_amd", "csrc"), SRC, obj, "-lpthread",
                    "-o", exe], check=True)
    return exe


def _run(exe, first, count, env=None):
    r = subprocess.run([exe, str(first), str(count)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert f"{count} seeds, 0 failed, 0 contract violations" in r.stdout
    # the mixes must reach every branch, or the fuzz passes without running it: copies that span
    # batches and whole ones, batches with one id to share, ids that serve a second copy, parts
    # with damaged copies and with chunks of several locations
    counts = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout))
    for what in ("batches", "continued", "whole", "one_open", "reused_ids", "long_copies",
                 "damaged", "multi_location"):
        assert counts[what] > 0, r.stdout
    assert counts["batches"] > 20 * count and counts["entries"] > counts["batches"]


def test_verify_many_stream_host_loop_fuzz(tmp_path):
    _run(_build(tmp_path, "verify_many_stream_host_fuzz", ["-O1"]), 0, 400)


def test_verify_many_stream_host_loop_fuzz_under_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O0"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _run(_build(tmp_path, "verify_many_stream_host_fuzz_san", san), 9000, 100, env)
