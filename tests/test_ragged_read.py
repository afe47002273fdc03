"""Ragged read, the part that needs no GPU: every argument check of cec_reconstruct_ragged,
cec_read_ragged, cec_resilver_ragged and cec_parts_read, which all come before any device use,
in the order of the write side's checks (tests/test_ragged.py)."""
import ctypes

import pytest

import chunky_ec as ce

LENS = [1, 15, 16, 17, 683]
D, P = 3, 2
T = D + P
BASE = 1 << 20  # never dereferenced: every case below returns before any device use
FILL = 0xEE


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _u8(values):
    return (ctypes.c_uint8 * max(len(values), 1))(*values)


def _reconstruct(rs, base, offs, lens, present=None, n=None, data_only=0, null=()):
    """Raw cec_reconstruct_ragged; `null` names the pointer arguments passed as NULL."""
    if present is None:
        present = ([0] + [1] * (T - 1)) * len(lens)
    a_offs, a_lens, a_pres = _sz(offs), _sz(lens), _u8(present)
    return ce._lib.cec_reconstruct_ragged(
        None if "codec" in null else rs.handle,
        None if "base" in null else base,
        None if "offs" in null else a_offs,
        None if "lens" in null else a_lens,
        len(lens) if n is None else n,
        None if "present" in null else a_pres,
        data_only, None)


def _verify_rebuild(fn, rs, base, offs, lens, present=None, n=None, null=()):
    """Raw cec_read_ragged / cec_resilver_ragged -> (code, outputs untouched)."""
    count = len(lens)
    if present is None:
        present = ([0] + [1] * (T - 1)) * count
    a_offs, a_lens, a_pres = _sz(offs), _sz(lens), _u8(present)
    verified = _u8([FILL] * (count * T))
    status = (ctypes.c_int * max(count, 1))(*([77] * count))
    code = fn(
        None if "codec" in null else rs.handle,
        None if "base" in null else base,
        None if "offs" in null else a_offs,
        None if "lens" in null else a_lens,
        count if n is None else n,
        None if "present" in null else a_pres,
        None if "expected" in null else BASE + (1 << 16),
        None if "verified" in null else verified,
        None if "status" in null else status, None)
    untouched = (all(b == FILL for b in bytes(verified)[:count * T]) and
                 list(status)[:count] == [77] * count)
    return code, untouched


READ_FNS = [ce._lib.cec_read_ragged, ce._lib.cec_resilver_ragged]


def _layout_cases(offs):
    """(offsets, lengths, n or None) that must give ERR_INVALID_ARGUMENT, from the layout."""
    cases = []
    for k in range(len(LENS)):
        for delta in (1, 8, 15):  # an offset not a multiple of 16
            bad = list(offs)
            bad[k] += delta
            cases.append((bad, LENS, None))
    for k in range(1, len(LENS)):  # overlapping: off[k+1] < off[k] + (d+p) * stride(L_k)
        bad = list(offs)
        bad[k] -= 16
        cases.append((bad, LENS, None))
    cases.append(([offs[1], offs[0]], LENS[:2], None))  # descending
    cases.append(([0, 0], [16, 16], None))
    # counts beyond the kernels' 32-bit indices: more than 2^32 - 1 chunks (n_parts itself is
    # checked before the arrays are read), a part that overflows size_t, more work units than
    # one grid can hold
    cases.append(([0], [16], (1 << 32) // T + 1))
    cases.append(([0], [2 ** 62], None))
    cases.append(([0], [2 ** 64 - 1], None))
    cases.append(([0], [1 << 50], None))
    return cases


def test_reconstruct_ragged_argument_errors_precede_device_use():
    rs = ce.ReedSolomon(D, P)
    offs, _ = ce.ragged_layout(T, LENS)
    for null in ("codec", "base", "offs", "lens", "present"):
        assert _reconstruct(rs, BASE, offs, LENS, null=(null,)) == ce.ERR_INVALID_ARGUMENT, null
    for k in range(len(LENS)):
        lens = list(LENS)
        lens[k] = 0
        assert _reconstruct(rs, BASE, offs, lens) == ce.EMPTY_SHARD
    for b in (BASE + 1, BASE + 8, BASE + 15):
        assert _reconstruct(rs, b, offs, LENS) == ce.ERR_INVALID_ARGUMENT
    for bad_offs, lens, n in _layout_cases(offs):
        pres = [1] * (T * len(lens))
        assert _reconstruct(rs, BASE, bad_offs, lens, present=pres, n=n) == \
            ce.ERR_INVALID_ARGUMENT, (bad_offs, lens, n)
    # a zero length wins over a bad layout behind it, as in ragged_check
    lens = list(LENS)
    lens[0] = 0
    assert _reconstruct(rs, BASE + 1, offs, lens) == ce.EMPTY_SHARD


@pytest.mark.parametrize("data_only", [0, 1])
def test_reconstruct_ragged_too_few_present(data_only):
    rs = ce.ReedSolomon(D, P)
    offs, _ = ce.ragged_layout(T, LENS)
    good = [1] * T
    for k in range(len(LENS)):
        for n_present in range(1, D):
            pres = good * len(LENS)
            pres[k * T:(k + 1) * T] = [1] * n_present + [0] * (T - n_present)
            assert _reconstruct(rs, BASE, offs, LENS, present=pres, data_only=data_only) == \
                ce.TOO_FEW_SHARDS_PRESENT, (k, n_present)
    # the layout is checked first
    pres = good * len(LENS)
    pres[0:T] = [1] + [0] * (T - 1)
    assert _reconstruct(rs, BASE + 1, offs, LENS, present=pres) == ce.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("fn", READ_FNS, ids=["read", "resilver"])
def test_read_ragged_argument_errors_precede_device_use(fn):
    rs = ce.ReedSolomon(D, P)
    offs, _ = ce.ragged_layout(T, LENS)
    for null in ("codec", "base", "offs", "lens", "present", "expected", "verified", "status"):
        code, untouched = _verify_rebuild(fn, rs, BASE, offs, LENS, null=(null,))
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, null
    for k in range(len(LENS)):
        lens = list(LENS)
        lens[k] = 0
        code, untouched = _verify_rebuild(fn, rs, BASE, offs, lens)
        assert code == ce.EMPTY_SHARD and untouched
    for b in (BASE + 1, BASE + 8, BASE + 15):
        code, untouched = _verify_rebuild(fn, rs, b, offs, LENS)
        assert code == ce.ERR_INVALID_ARGUMENT and untouched
    for bad_offs, lens, n in _layout_cases(offs):
        code, untouched = _verify_rebuild(fn, rs, BASE, bad_offs, lens, n=n)
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, (bad_offs, lens, n)


def _parts_read_raw(rs, lens, present, data_only=1, null=(), null_slots=()):
    """Raw cec_parts_read over 0xEE-filled slots -> (code, everything untouched).  `null_slots`
    lists (k, i) passed as NULL chunk pointers."""
    n = len(lens)
    slots = [(ctypes.c_uint8 * max(lens[k], 1))() for k in range(n) for _ in range(T)]
    for s in slots:
        ctypes.memset(s, FILL, len(s))
    ptrs = (ce._u8p * max(n * T, 1))(*[
        ce._u8p() if (q // T, q % T) in null_slots else ctypes.cast(s, ce._u8p)
        for q, s in enumerate(slots)])
    expected = _u8([0] * (n * T * 32))
    verified = _u8([FILL] * (n * T))
    status = (ctypes.c_int * max(n, 1))(*([77] * n))
    code = ce._lib.cec_parts_read(
        None if "codec" in null else rs.handle,
        None if "shards" in null else ptrs,
        None if "lens" in null else _sz(lens), n,
        None if "present" in null else _u8(present),
        None if "expected" in null else expected,
        data_only,
        None if "verified" in null else verified,
        None if "status" in null else status)
    untouched = (all(b == FILL for s in slots for b in bytes(s)) and
                 all(b == FILL for b in bytes(verified)[:n * T]) and
                 list(status)[:n] == [77] * n)
    return code, untouched


def test_parts_read_argument_errors_precede_device_use():
    rs = ce.ReedSolomon(D, P)
    lens = [7, 20480, 1]
    present = ([0] + [1] * (T - 1)) * 3
    for null in ("codec", "shards", "lens", "present", "expected", "verified", "status"):
        code, untouched = _parts_read_raw(rs, lens, present, null=(null,))
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, null
    # a zero length anywhere in the list: EmptyShard before anything is written
    for k in range(3):
        bad = list(lens)
        bad[k] = 0
        code, untouched = _parts_read_raw(rs, bad, present)
        assert code == ce.EMPTY_SHARD and untouched, k
    # a slot that must be filled and is NULL: the missing data chunk; under resilver the
    # missing parity chunk too; a loaded chunk without bytes
    code, untouched = _parts_read_raw(rs, lens, present, null_slots=((1, 0),))
    assert code == ce.ERR_INVALID_ARGUMENT and untouched
    par_missing = [1] * (T - 1) + [0]
    code, untouched = _parts_read_raw(rs, [16], par_missing, data_only=0, null_slots=((0, T - 1),))
    assert code == ce.ERR_INVALID_ARGUMENT and untouched
    code, untouched = _parts_read_raw(rs, lens, present, null_slots=((2, 3),))
    assert code == ce.ERR_INVALID_ARGUMENT and untouched
    # ... while a read never fills missing parity: NULL there is no argument error
    code, untouched = _parts_read_raw(rs, [16], par_missing, data_only=1, null_slots=((0, T - 1),))
    assert code != ce.ERR_INVALID_ARGUMENT
    if ce.device_count() == 0:
        assert code == ce.ERR_NO_DEVICE and untouched
    # the Python wrapper reports a zero chunk length the same way
    with pytest.raises(ce.Error) as e:
        ce.parts_read(rs, [[b"", b"", b"", None, None]], [[b"\0" * 32] * T])
    assert e.value.code == ce.EMPTY_SHARD


def test_ragged_read_zero_parts_is_ok():
    rs = ce.ReedSolomon(D, P)
    assert _reconstruct(rs, BASE, [], [], present=[], n=0) == ce.OK
    assert ce._lib.cec_reconstruct_ragged(rs.handle, None, None, None, 0, None, 0, None) == ce.OK
    for fn in READ_FNS:
        assert fn(rs.handle, None, None, None, 0, None, None, None, None, None) == ce.OK
    assert ce._lib.cec_parts_read(rs.handle, None, None, 0, None, None, 1, None, None) == ce.OK
    ce.reconstruct_ragged(rs, 0, [], [], b"", True)
    assert ce.read_ragged(rs, 0, [], [], b"", 0) == (b"", [])
    assert ce.resilver_ragged(rs, 0, [], [], b"", 0) == (b"", [])
    assert ce.parts_read(rs, [], []) == ([], b"", [])


def test_ragged_read_without_a_device():
    """Well-formed calls on a machine without a GPU: ERR_NO_DEVICE, outputs untouched.  (With a
    device the GPU suite runs these calls on real memory.)"""
    if ce.device_count() != 0:
        return
    rs = ce.ReedSolomon(D, P)
    offs, _ = ce.ragged_layout(T, LENS)
    spaced = [o + 4096 * k for k, o in enumerate(offs)]
    for o in (offs, spaced):
        assert _reconstruct(rs, BASE, o, LENS) == ce.ERR_NO_DEVICE
        assert _reconstruct(rs, BASE, o, LENS, present=[1] * (T * len(LENS))) == ce.ERR_NO_DEVICE
        for fn in READ_FNS:
            code, untouched = _verify_rebuild(fn, rs, BASE, o, LENS)
            assert code == ce.ERR_NO_DEVICE and untouched
    code, untouched = _parts_read_raw(rs, [7, 20480, 1], ([0] + [1] * (T - 1)) * 3)
    assert code == ce.ERR_NO_DEVICE and untouched
