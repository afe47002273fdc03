"""The fused ragged encode, the part that needs no GPU: cec_ragged_stats is declared, exported and
bound, and with CEC_RAGGED_FUSED=1 the argument errors of cec_encode_hash_ragged and
cec_encode_hash_split still come in their order and before any device use."""
import ctypes
import os
import re
import subprocess
import sys

import chunky_ec as ce
import test_ragged
import test_split
from test_ragged import _ragged
from test_split import BASE_D, _split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "chunky-bits_amd", "chunky_ec", "libchunky_ec.so")


def _declares(header, name):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.search(r"\b%s\s*\(" % name, src) is not None


def test_ragged_stats_is_declared_exported_and_bound():
    assert _declares("chunky_ec.h", "cec_ragged_stats")
    assert not _declares("chunky_ec_parts.h", "cec_ragged_stats")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r" T cec_ragged_stats\b", out)
    rust = open(os.path.join(ROOT, "chunky-bits_amd", "rust", "chunky-ec-sys", "src",
                             "lib.rs")).read()
    assert "pub fn cec_ragged_stats(fused: *mut u64, two_pass: *mut u64);" in rust
    assert "pub fn ragged_stats() -> (u64, u64)" in rust
    assert ce.abi_version() == 3  # additive
    fused, two_pass = ce.ragged_stats()
    assert isinstance(fused, int) and isinstance(two_pass, int)


def test_ragged_stats_tolerates_null_pointers():
    lib = ce._lib
    f, s = ctypes.c_uint64(7), ctypes.c_uint64(7)
    lib.cec_ragged_stats(None, None)
    lib.cec_ragged_stats(ctypes.byref(f), None)
    lib.cec_ragged_stats(None, ctypes.byref(s))
    assert (f.value, s.value) == ce.ragged_stats()


def test_ragged_stats_is_zero_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); import chunky_ec as ce; "
            "print(ce.ragged_stats())" % os.path.join(ROOT, "chunky-bits_amd"))
    for knob in (None, "0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "CEC_RAGGED_FUSED"}
        if knob is not None:
            env["CEC_RAGGED_FUSED"] = knob
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                             check=True, env=env).stdout
        assert out.strip() == "(0, 0)", (knob, out)


def test_argument_errors_keep_their_order_with_the_fused_path_forced(knob_env):
    """Every case of the two-pass path's own argument tests, run again with CEC_RAGGED_FUSED=1:
    the choice of path comes behind every check, so nothing moves.  Without a GPU the sound calls
    at their ends report NoDevice, and no launch sequence is ever counted."""
    before = ce.ragged_stats()
    for value in ("1", "0"):
        knob_env.set("CEC_RAGGED_FUSED", value)
        test_ragged.test_encode_hash_ragged_argument_errors_precede_device_use()
        test_split.test_encode_hash_split_argument_errors_in_order()
        rs = ce.ReedSolomon(3, 2)
        # a null pointer beside a zero length beside a misaligned base: the null pointer wins,
        # then the zero length, then the base
        assert _ragged(rs, (1 << 20) + 1, [0], [0], null=("digests",)) == ce.ERR_INVALID_ARGUMENT
        assert _ragged(rs, (1 << 20) + 1, [0], [0]) == ce.EMPTY_SHARD
        assert _ragged(rs, (1 << 20) + 1, [0], [16]) == ce.ERR_INVALID_ARGUMENT
        assert _split(rs, [0], [0], [0], dbase=BASE_D + 1, null=("poffs",)) == \
            ce.ERR_INVALID_ARGUMENT
        assert _split(rs, [0], [0], [0], dbase=BASE_D + 1) == ce.EMPTY_SHARD
        # a chunk the fused kernel's 32-bit step count could not walk is refused as before
        # (more work units than one grid holds), not handed to it
        assert _ragged(rs, 1 << 20, [0], [1 << 50]) == ce.ERR_INVALID_ARGUMENT
    if ce.device_count() == 0:
        assert ce.ragged_stats() == before
