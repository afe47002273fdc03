"""The ragged tier's word layouts (csrc/ragged_words.hpp): where the words of a ragged encode, a
verification, an async read and a reconstruct lie in their scratch buffers, and the pure host
functions that fill them (part_records, length_order, sha_list).  The host compiles the header
without the HIP runtime; tests/cpp/ragged_words_test.cpp checks it on the CPU over seeded random
batches, plain and under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chunky-bits_amd", "csrc")


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_ragged_words_rules_hold_over_random_batches():
    """The program the library's build leaves beside its source."""
    exe = os.path.join(ROOT, "tests", "cpp", "ragged_words_test")
    assert os.path.exists(exe), "build() makes tests/cpp/ragged_words_test"
    r = _run([exe])
    assert r.returncode == 0 and "ragged_words ok: 120 random batches" in r.stdout, r.stdout


def test_ragged_words_rules_under_sanitizers(tmp_path):
    """The same program (host code only, its own main) built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "ragged_words_san")
    r = _run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=undefined", "-I", CSRC,
              os.path.join(ROOT, "tests", "cpp", "ragged_words_test.cpp"), "-o", exe])
    assert r.returncode == 0, r.stdout
    r = _run([exe])
    assert r.returncode == 0 and "ragged_words ok" in r.stdout, r.stdout
