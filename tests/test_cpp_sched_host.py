"""The scheduler (csrc/multi.cpp), the write and read pipelines (csrc/pipeline.cpp) and the pinned
registry (csrc/hostmem.cpp) on the CPU: tests/cpp/sched_host_test.cpp links those sources, and
knobs.cpp, UNCHANGED against a host stand-in of the HIP runtime (tests/cpp/hip_standin/: streams
are threads with seeded delays, events capture a position, misuse is recorded) and compute
stand-ins backed by the oracle (tests/cpp/sched_host_compute.cpp).  The program runs its
self-test and scenarios a to e (write pipeline, read pipeline and carry pool, scheduler, lifecycle,
creation failures) and asserts after each that the results are the oracle's, no canary is touched,
the stand-in saw no violation and no hazard, nothing is left live and every slot carried a batch.
Built and run plain, under ThreadSanitizer and under AddressSanitizer +
UndefinedBehaviorSanitizer (stand-alone programs: host code only); two mutants of the stand-in
(an event wait that does not wait, a dropped stream-wait-event) must make it fail."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chunky-bits_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
SOURCES = [os.path.join(CPP, "sched_host_test.cpp"), os.path.join(CPP, "sched_host_compute.cpp"),
           os.path.join(CPP, "hip_standin", "standin.cpp")] + [
               os.path.join(CSRC, f) for f in ("pipeline.cpp", "multi.cpp", "hostmem.cpp", "knobs.cpp")]
INCLUDES = ["-I", os.path.join(CPP, "hip_standin"), "-I", CPP, "-I", os.path.join(ROOT, "include"),
            "-I", CSRC]


def _build(tmp, name, flags):
    if not (shutil.which("gcc") and shutil.which("g++")):
        pytest.skip("no host compiler")
    jobs = [["gcc", *flags, "-c", os.path.join(ROOT, "oracle", "cec_oracle.c"), "-o",
             str(tmp / (name + "_oracle.o"))]]
    objs = [jobs[0][-1]]
    for i, src in enumerate(SOURCES):
        objs.append(str(tmp / f"{name}_{i}.o"))
        jobs.append(["g++", "-std=c++17", "-Wall", "-Werror", *flags, *INCLUDES, "-c", src, "-o",
                     objs[-1]])
    with ThreadPoolExecutor(max_workers=4) as pool:  # the sources compile side by side
        for r in pool.map(lambda j: subprocess.run(j, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-4000:]
    exe = str(tmp / name)
    subprocess.run(["g++", *flags, *objs, "-lpthread", "-o", exe], check=True)
    return exe


def _run(exe, first, count, env=None):
    return subprocess.run([exe, str(first), str(count)], capture_output=True, text=True,
                          timeout=300, env=env)


def _passes(r, count):
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-8000:]
    assert "selftest: ok" in r.stdout
    assert f"sched_host_test: {count} seeds" in r.stdout and ", 0 failed" in r.stdout
    # every constructor had each of its creating calls failed once
    assert r.stdout.count("creating calls, each failed once") == 6, r.stdout


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sched_host"), "sched_host_test", ["-O1"])


def test_sched_host(plain):
    _passes(_run(plain, 1, 12), 12)


def test_sched_host_under_thread_sanitizer(tmp_path):
    exe = _build(tmp_path, "sched_host_test_tsan", ["-fsanitize=thread", "-g", "-O1"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    _passes(_run(exe, 100, 2, env), 2)


def test_sched_host_under_address_and_ub_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = _build(tmp_path, "sched_host_test_asan", san)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    _passes(_run(exe, 200, 2, env), 2)


@pytest.mark.parametrize("mutant", ["event_sync", "stream_wait"])
def test_sched_host_notices_a_missing_wait(plain, mutant):
    """hipEventSynchronize returning without waiting, and hipStreamWaitEvent dropped: the program
    must end non-zero and name a result mismatch or a stand-in violation."""
    r = _run(plain, 1, 1, dict(os.environ, SCHED_HOST_MUTANT=mutant))
    assert r.returncode != 0, r.stdout[-2000:]
    assert "FAILED" in r.stdout and ("result mismatch" in r.stdout or "violation" in r.stdout), \
        r.stdout[-2000:]
