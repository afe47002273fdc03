"""The segmented scrub's pure host pieces (csrc/scrub_words.hpp): the word layout of the verifying
resume launch (the resume list of one chunk per part, the expected rows and the ok bytes behind it
where the scrub pipeline's one upload wants them), the record indices, the filled list and the
entry rules of cec_verify_segments in their order.  The host compiles the header without the HIP
runtime; tests/cpp/scrub_words_test.cpp checks it on the CPU over seeded random entry lists, plain
and under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chunky-bits_amd", "csrc")


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_scrub_words_rules_hold_over_random_entry_lists():
    """The program the library's build leaves beside its source."""
    exe = os.path.join(ROOT, "tests", "cpp", "scrub_words_test")
    assert os.path.exists(exe), "build() makes tests/cpp/scrub_words_test"
    r = _run([exe])
    assert r.returncode == 0 and "scrub_words ok: 4000 random entry lists" in r.stdout, r.stdout


def test_scrub_words_rules_under_sanitizers(tmp_path):
    """The same program (host code only, its own main) built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "scrub_words_san")
    r = _run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=undefined", "-I", CSRC,
              os.path.join(ROOT, "tests", "cpp", "scrub_words_test.cpp"), "-o", exe])
    assert r.returncode == 0, r.stdout
    r = _run([exe])
    assert r.returncode == 0 and "scrub_words ok" in r.stdout, r.stdout
