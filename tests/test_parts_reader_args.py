"""The ragged read with a packed return and the parts reader, the part that needs no GPU: every
argument check of cec_read_ragged_packed_async and cec_parts_reader_new comes before any device
use, in the order include/chunky_ec_parts_read.h states, and leaves the outputs untouched; the
reader's calls refuse a null handle; and the packed return's offset rule (csrc/return_plan.hpp),
which the kernel and the host compile alike, agrees with a plain loop on the CPU
(tests/cpp/return_plan_test.cpp), plain and under the address and undefined-behaviour sanitizers.
(The submits' checks need a reader, hence a device: tests/test_gpu_parts_reader.py.)"""
import ctypes
import os
import shutil
import subprocess

import pytest

import chunky_ec as ce
from test_ragged_read import BASE, D, LENS, P, T, _layout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chunky-bits_amd", "csrc")
REGION = 1 << 31  # never dereferenced
FILL = 0xEE


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _stride(L):
    return (L + 15) // 16 * 16


def _worst(d, p, data_only, lens):
    return sum((min(p, d) if data_only else p) * _stride(L) for L in lens)


def _packed(rs, base, offs, lens, data_only=1, n=None, null=(), rebuilt=REGION, cap=None):
    """Raw cec_read_ragged_packed_async; `null` names the pointer arguments passed as NULL.
    Returns (code, whether verified, part_status and rebuilt_offsets are untouched)."""
    count = len(lens) if n is None else n
    items = len(lens) * T
    pres = (ctypes.c_uint8 * max(items, 1))(*([1] * items))
    ver = (ctypes.c_uint8 * max(items, 1))(*([FILL] * max(items, 1)))
    st = (ctypes.c_int * max(len(lens), 1))(*([FILL] * max(len(lens), 1)))
    off = (ctypes.c_size_t * (len(lens) + 1))(*([FILL] * (len(lens) + 1)))
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    if cap is None:
        cap = _worst(d, p, data_only, [L for L in lens if L < 2 ** 40])
    code = ce._lib.cec_read_ragged_packed_async(
        None if "codec" in null else rs.handle,
        None if "base" in null else base,
        None if "offs" in null else _sz(offs),
        None if "lens" in null else _sz(lens),
        count,
        None if "present" in null else pres,
        None if "expected" in null else BASE,
        data_only,
        None if "verified" in null else ver,
        None if "status" in null else st,
        None if "rebuilt" in null else rebuilt,
        cap,
        None if "offsets" in null else off,
        None)
    untouched = all(v == FILL for v in ver) and all(v == FILL for v in st) and \
        all(v == FILL for v in off)
    return code, untouched


@pytest.mark.parametrize("data_only", [1, 0], ids=["data_only", "all"])
def test_packed_argument_errors_precede_device_use_in_order(data_only):
    rs = ce.ReedSolomon(D, P)
    offs, _ = ce.ragged_layout(T, LENS)
    # 1. null pointers, the two new ones among them, even beside every later error
    for null in ("codec", "base", "offs", "lens", "present", "expected", "verified", "status",
                 "rebuilt", "offsets"):
        assert _packed(rs, BASE, offs, LENS, data_only, null=(null,)) == \
            (ce.ERR_INVALID_ARGUMENT, True), null
        assert _packed(rs, BASE + 1, offs, [0] + LENS[1:], data_only, null=(null,), cap=0) == \
            (ce.ERR_INVALID_ARGUMENT, True), null
    # 2. cec_read_ragged_async's checks, in its order: a zero length wins over a bad base, a bad
    #    region and a small cap
    for k in range(len(LENS)):
        lens = list(LENS)
        lens[k] = 0
        for kw in ({}, {"rebuilt": REGION + 8}, {"cap": 0}):
            assert _packed(rs, BASE + 1, offs, lens, data_only, **kw) == (ce.EMPTY_SHARD, True)
    for b in (BASE + 1, BASE + 8, BASE + 15):
        assert _packed(rs, b, offs, LENS, data_only) == (ce.ERR_INVALID_ARGUMENT, True)
    for bad_offs, lens, n in _layout_cases(offs):
        assert _packed(rs, BASE, bad_offs, lens, data_only, n=n) == \
            (ce.ERR_INVALID_ARGUMENT, True), (bad_offs, lens, n)
    # 3. the region: 16-byte aligned
    for delta in (1, 8, 15):
        assert _packed(rs, BASE, offs, LENS, data_only, rebuilt=REGION + delta) == \
            (ce.ERR_INVALID_ARGUMENT, True)
    # 4. a cap below the worst case, by one column and by everything; the reason is given
    worst = _worst(D, P, data_only, LENS)
    for cap in (worst - 16, worst - 1, 0):
        assert _packed(rs, BASE, offs, LENS, data_only, cap=cap) == (ce.ERR_INVALID_ARGUMENT, True)
        assert b"rebuilt_cap" in ce._lib.cec_last_error()
    # 5. sound arguments: the device is looked for only now
    if ce.device_count() == 0:
        before = ce.ragged_read_stats()
        assert _packed(rs, BASE, offs, LENS, data_only, cap=worst) == (ce.ERR_NO_DEVICE, True)
        assert _packed(rs, BASE, offs, LENS, data_only, cap=worst + 1) == (ce.ERR_NO_DEVICE, True)
        assert ce.ragged_read_stats() == before


@pytest.mark.parametrize("d,p", [(4, 9), (33, 2), (40, 9)])
def test_packed_refuses_shapes_outside_the_planner(d, p):
    rs = ce.ReedSolomon(d, p)
    t = d + p
    lens = [16, 17, 4097]
    offs, _ = ce.ragged_layout(t, lens)
    for data_only in (1, 0):
        items = len(lens) * t
        pres = (ctypes.c_uint8 * items)(*([1] * items))
        ver = (ctypes.c_uint8 * items)(*([FILL] * items))
        st = (ctypes.c_int * 3)(FILL, FILL, FILL)
        off = (ctypes.c_size_t * 4)(FILL, FILL, FILL, FILL)
        code = ce._lib.cec_read_ragged_packed_async(
            rs.handle, BASE, _sz(offs), _sz(lens), 3, pres, BASE, data_only, ver, st, REGION,
            1 << 30, off, None)
        assert code == ce.ERR_INVALID_ARGUMENT
        assert b"planner" in ce._lib.cec_last_error()
        assert all(v == FILL for v in ver) and all(v == FILL for v in st) and \
            all(v == FILL for v in off)
    # the reader refuses them when it is made
    out = ce._vp()
    assert ce._lib.cec_parts_reader_new(rs.handle, 1 << 20, 64, 2, 1, ctypes.byref(out)) == \
        ce.ERR_INVALID_ARGUMENT
    assert b"planner" in ce._lib.cec_last_error() and not out


def test_packed_zero_parts_is_a_batch_of_nothing():
    rs = ce.ReedSolomon(D, P)
    fn = ce._lib.cec_read_ragged_packed_async
    off = (ctypes.c_size_t * 1)(FILL)
    assert fn(rs.handle, None, None, None, 0, None, None, 1, None, None, None, 0, off, None) == \
        ce.OK
    assert off[0] == 0
    assert fn(rs.handle, None, None, None, 0, None, None, 0, None, None, None, 0, None, None) == \
        ce.OK
    assert fn(None, None, None, None, 0, None, None, 1, None, None, None, 0, off, None) == \
        ce.ERR_INVALID_ARGUMENT
    buf = bytearray(8)
    ce.read_ragged_packed_async(rs, 0, [], [], b"", 0, True, bytearray(1), bytearray(4), 0, 0, buf)
    assert buf == bytes(8)


def test_packed_wrapper_refuses_short_outputs():
    rs = ce.ReedSolomon(D, P)
    offs, _ = ce.ragged_layout(T, [16, 16])
    pres = bytes([1] * (2 * T))
    good = (bytearray(2 * T), bytearray(8), bytearray(24))
    for i, short in enumerate((bytearray(2 * T - 1), bytearray(7), bytearray(23))):
        bufs = list(good)
        bufs[i] = short
        with pytest.raises(ValueError):
            ce.read_ragged_packed_async(rs, BASE, offs, [16, 16], pres, BASE, True, bufs[0],
                                        bufs[1], REGION, 1 << 20, bufs[2])


def test_parts_reader_new_errors_in_order():
    rs = ce.ReedSolomon(3, 2)
    lib, out = ce._lib, ce._vp()
    new = lib.cec_parts_reader_new
    assert new(None, 1 << 20, 64, 2, 1, ctypes.byref(out)) == ce.ERR_INVALID_ARGUMENT
    assert new(rs.handle, 1 << 20, 64, 2, 1, None) == ce.ERR_INVALID_ARGUMENT
    # the sizes, before the device is looked for
    for slot_bytes, max_parts, depth in ((1 << 20, 64, 0), (1 << 20, 64, 17), (1 << 20, 0, 2),
                                         (5 * 16 - 1, 64, 2), (0, 64, 2), (2 ** 64 - 1, 64, 2),
                                         (1 << 20, 2 ** 60, 2), (1 << 20, (1 << 32) // 5 + 1, 2)):
        for data_only in (1, 0):
            assert new(rs.handle, slot_bytes, max_parts, depth, data_only, ctypes.byref(out)) == \
                ce.ERR_INVALID_ARGUMENT, (slot_bytes, max_parts, depth)
            assert not out
    assert b"slot_bytes" in lib.cec_last_error()
    with pytest.raises(ce.Error) as e:
        ce.PartsReader(rs, 1 << 20, 64, 0)
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    if ce.device_count() == 0:
        assert new(rs.handle, 5 * 16, 1, 1, 1, ctypes.byref(out)) == ce.ERR_NO_DEVICE
        assert new(rs.handle, 1 << 20, 64, 16, 0, ctypes.byref(out)) == ce.ERR_NO_DEVICE
        with pytest.raises(ce.Error) as e:
            ce.PartsReader(rs, 1 << 20, 64, 2)
        assert e.value.code == ce.ERR_NO_DEVICE


def test_parts_reader_calls_refuse_a_null_reader():
    lib = ce._lib
    slot, ptr, n = ctypes.c_size_t(0), ce._u8p(), ctypes.c_size_t(0)
    st, off = ctypes.POINTER(ctypes.c_int)(), ce._szp()
    bufs = (ce._u8p * 5)()
    flags, exp = (ctypes.c_uint8 * 5)(), (ctypes.c_uint8 * 160)()
    assert lib.cec_parts_reader_depth(None) == 0
    assert lib.cec_parts_reader_acquire(None, ctypes.byref(slot), ctypes.byref(ptr)) == \
        ce.ERR_INVALID_ARGUMENT
    for lens in ([16], [0]):  # a null reader wins over a zero length
        assert lib.cec_parts_reader_submit(None, 0, _sz(lens), 1, flags, exp) == \
            ce.ERR_INVALID_ARGUMENT
        assert lib.cec_parts_reader_submit_from(None, 0, bufs, _sz(lens), 1, flags, exp) == \
            ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_wait(None, 0, ctypes.byref(ptr), ctypes.byref(st),
                                     ctypes.byref(ptr), ctypes.byref(off), ctypes.byref(n)) == \
        ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_scatter(None, 0, bufs) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_query(None, 0) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_drain(None) == ce.ERR_INVALID_ARGUMENT
    up, down, tails = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    lib.cec_parts_reader_stats(None, ctypes.byref(up), ctypes.byref(down), ctypes.byref(tails))
    assert (up.value, down.value, tails.value) == (0, 0, 0)
    lib.cec_parts_reader_stats(None, None, None, None)
    lib.cec_parts_reader_free(None)


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_return_plan_rule_agrees_with_a_plain_loop():
    """The program the library's build leaves beside its source."""
    exe = os.path.join(ROOT, "tests", "cpp", "return_plan_test")
    assert os.path.exists(exe), "build() makes tests/cpp/return_plan_test"
    r = _run([exe])
    assert r.returncode == 0 and "return_plan ok: 120 random batches" in r.stdout, r.stdout


def test_return_plan_rule_under_sanitizers(tmp_path):
    """The same program (host code only, its own main) built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "return_plan_san")
    r = _run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=undefined", "-I", CSRC,
              os.path.join(ROOT, "tests", "cpp", "return_plan_test.cpp"), "-o", exe])
    assert r.returncode == 0, r.stdout
    r = _run([exe])
    assert r.returncode == 0 and "return_plan ok" in r.stdout, r.stdout
