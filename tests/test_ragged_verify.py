"""Ragged verify, the part that needs no GPU: every argument check of cec_verify_ragged and
cec_parts_verify, which all come before any device use, in the order of cec_read_ragged's checks
(tests/test_ragged_read.py)."""
import ctypes

import pytest

import chunky_ec as ce
from test_ragged_read import _layout_cases

LENS = [1, 15, 16, 17, 683]
T = 5  # the shape _layout_cases is written for
BASE = 1 << 20  # never dereferenced: every case below returns before any device use
FILL = 0xEE


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _u8(values):
    return (ctypes.c_uint8 * max(len(values), 1))(*values)


def _verify(t, base, offs, lens, present="all", n=None, null=()):
    """Raw cec_verify_ragged -> (code, verified untouched).  present: "all" = every chunk
    flagged 1, None = a NULL pointer (every chunk present), or the flags."""
    count = len(lens)
    if present == "all":
        present = [1] * (count * t)
    a_offs, a_lens = _sz(offs), _sz(lens)
    a_pres = None if present is None else _u8(present)
    verified = _u8([FILL] * (count * t))
    code = ce._lib.cec_verify_ragged(
        t,
        None if "base" in null else base,
        None if "offs" in null else a_offs,
        None if "lens" in null else a_lens,
        count if n is None else n,
        a_pres,
        None if "expected" in null else BASE + (1 << 16),
        None if "verified" in null else verified, None)
    return code, all(b == FILL for b in bytes(verified)[:count * t])


def test_verify_ragged_argument_errors_precede_device_use():
    offs, _ = ce.ragged_layout(T, LENS)
    for null in ("base", "offs", "lens", "expected", "verified"):
        code, untouched = _verify(T, BASE, offs, LENS, null=(null,))
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, null
    code, untouched = _verify(0, BASE, offs, LENS)
    assert code == ce.ERR_INVALID_ARGUMENT and untouched
    for t in (T, 1):
        o, _ = ce.ragged_layout(t, LENS)
        for k in range(len(LENS)):
            lens = list(LENS)
            lens[k] = 0
            code, untouched = _verify(t, BASE, o, lens)
            assert code == ce.EMPTY_SHARD and untouched, (t, k)
    for b in (BASE + 1, BASE + 8, BASE + 15):
        code, untouched = _verify(T, b, offs, LENS)
        assert code == ce.ERR_INVALID_ARGUMENT and untouched
    for bad_offs, lens, n in _layout_cases(offs):
        for present in ("all", None):
            code, untouched = _verify(T, BASE, bad_offs, lens, present=present, n=n)
            assert code == ce.ERR_INVALID_ARGUMENT and untouched, (bad_offs, lens, n)
    # a zero length wins over a bad layout behind it, as in ragged_check
    lens = list(LENS)
    lens[0] = 0
    code, untouched = _verify(T, BASE + 1, offs, lens)
    assert code == ce.EMPTY_SHARD and untouched
    bad = list(offs)
    bad[2] += 8
    lens = list(LENS)
    lens[4] = 0
    code, untouched = _verify(T, BASE, bad, lens)
    assert code == ce.EMPTY_SHARD and untouched


def _parts_verify_raw(lens, null=(), null_bufs=(), n=None):
    """Raw cec_parts_verify over 0xEE-filled copies -> (code, ok untouched)."""
    count = len(lens)
    copies = [(ctypes.c_uint8 * max(ln, 1))() for ln in lens]
    for c in copies:
        ctypes.memset(c, FILL, len(c))
    ptrs = (ce._u8p * max(count, 1))(*[
        ce._u8p() if i in null_bufs else ctypes.cast(c, ce._u8p) for i, c in enumerate(copies)])
    expected = _u8([0] * (count * 32))
    ok = _u8([FILL] * count)
    code = ce._lib.cec_parts_verify(
        None if "bufs" in null else ptrs,
        None if "lens" in null else _sz(lens),
        count if n is None else n,
        None if "expected" in null else expected,
        None if "ok" in null else ok)
    return code, all(b == FILL for b in bytes(ok)[:count])


def test_parts_verify_argument_errors_precede_device_use():
    lens = [7, 20480, 1, 683]
    for null in ("bufs", "lens", "expected", "ok"):
        code, untouched = _parts_verify_raw(lens, null=(null,))
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, null
    # a zero length anywhere in the list: EmptyShard before anything is written
    for k in range(len(lens)):
        bad = list(lens)
        bad[k] = 0
        code, untouched = _parts_verify_raw(bad)
        assert code == ce.EMPTY_SHARD and untouched, k
    # a NULL copy; a zero length wins over it wherever the two stand
    for k in range(len(lens)):
        code, untouched = _parts_verify_raw(lens, null_bufs=(k,))
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, k
    code, untouched = _parts_verify_raw([7, 16, 0, 1], null_bufs=(0,))
    assert code == ce.EMPTY_SHARD and untouched
    # more copies than the 32-bit item index: refused before the arrays are walked
    code, untouched = _parts_verify_raw(lens, n=1 << 32)
    assert code == ce.ERR_INVALID_ARGUMENT and untouched
    # the Python wrapper reports a zero length the same way, and checks its own arguments
    with pytest.raises(ce.Error) as e:
        ce.parts_verify([b"abc", b""], [b"\0" * 32] * 2)
    assert e.value.code == ce.EMPTY_SHARD
    with pytest.raises(ValueError):
        ce.parts_verify([b"abc"], [])
    with pytest.raises(ValueError):
        ce.parts_verify([b"abc"], [b"\0" * 31])


def test_ragged_verify_zero_parts_is_ok():
    assert _verify(T, BASE, [], [], n=0) == (ce.OK, True)
    assert ce._lib.cec_verify_ragged(T, None, None, None, 0, None, None, None, None) == ce.OK
    # ... but not with no chunks per part
    assert ce._lib.cec_verify_ragged(0, None, None, None, 0, None, None, None, None) == \
        ce.ERR_INVALID_ARGUMENT
    assert ce._lib.cec_parts_verify(None, None, 0, None, None) == ce.OK
    assert ce.verify_ragged(T, 0, [], [], b"", 0) == b""
    assert ce.verify_ragged(1, 0, [], [], None, 0) == b""
    assert ce.parts_verify([], []) == b""


def test_ragged_verify_without_a_device():
    """Well-formed calls on a machine without a GPU: ERR_NO_DEVICE, outputs untouched; a NULL
    `present` is accepted as every chunk present.  (With a device the GPU suite runs these calls
    on real memory.)"""
    if ce.device_count() != 0:
        return
    for t in (T, 1, 14):
        offs, _ = ce.ragged_layout(t, LENS)
        spaced = [o + 4096 * k for k, o in enumerate(offs)]
        mixed = ([0, 1, ce.PRESENT_VERIFIED] * (t * len(LENS)))[:t * len(LENS)]
        for o in (offs, spaced):
            for present in ("all", None, mixed):
                code, untouched = _verify(t, BASE, o, LENS, present=present)
                assert code == ce.ERR_NO_DEVICE and untouched, (t, present)
    code, untouched = _parts_verify_raw([7, 20480, 1, 683])
    assert code == ce.ERR_NO_DEVICE and untouched
    with pytest.raises(ce.Error) as e:
        ce.parts_verify([b"abc"], [b"\0" * 32])
    assert e.value.code == ce.ERR_NO_DEVICE
