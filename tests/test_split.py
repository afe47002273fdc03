"""The split ragged layout and the parts pipeline, the part that needs no GPU: cec_split_layout
and every argument check of cec_encode_hash_split, cec_parts_pipeline_new and the submits, which
all come before any device use and in the order the header states."""
import ctypes

import pytest

import chunky_ec as ce

# tests/test_gpu_ragged.py LENGTHS (that module needs a GPU to import)
LENGTHS = [1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 683, 1023, 1024, 1025, 4095, 4096, 4097,
           8191, 8192, 8193, 16383, 16384, 16385, 65537]
BASE_D, BASE_P = 1 << 30, 1 << 20  # never dereferenced


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _stride(L):
    return (L + 15) // 16 * 16


def _split(rs, lens, doffs, poffs, dbase=BASE_D, pbase=BASE_P, n=None, null=()):
    """Raw cec_encode_hash_split; `null` names the pointer arguments passed as NULL."""
    a_d, a_p, a_l = _sz(doffs), _sz(poffs), _sz(lens)
    return ce._lib.cec_encode_hash_split(
        None if "codec" in null else rs.handle,
        None if "data" in null else dbase,
        None if "doffs" in null else a_d,
        None if "parity" in null else pbase,
        None if "poffs" in null else a_p,
        None if "lens" in null else a_l,
        len(lens) if n is None else n,
        None if "digests" in null else 16, None)


@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_split_layout_values(d, p):
    doffs, poffs, db, pb = ce.split_layout(d, p, LENGTHS)
    want_d, want_p, ad, ap = [], [], 0, 0
    for L in LENGTHS:
        want_d.append(ad)
        want_p.append(ap)
        ad += d * _stride(L)
        ap += p * _stride(L)
    assert (doffs, poffs, db, pb) == (want_d, want_p, ad, ap)
    assert all(o % 16 == 0 for o in doffs + poffs)
    assert ce.split_layout(d, p, []) == ([], [], 0, 0)
    # each region is the ragged layout of its own chunk count
    assert (doffs, db) == ce.ragged_layout(d, LENGTHS)
    assert (poffs, pb) == ce.ragged_layout(p, LENGTHS)


def test_split_layout_errors():
    for lens in ([0], [5, 0, 5]):
        with pytest.raises(ce.Error) as e:
            ce.split_layout(3, 2, lens)
        assert e.value.code == ce.EMPTY_SHARD
    for d, p in ((0, 2), (3, 0)):
        with pytest.raises(ce.Error) as e:
            ce.split_layout(d, p, [5])
        assert e.value.code == ce.ERR_INVALID_ARGUMENT
    for d, p in ((5, 1), (1, 5)):  # 5 * stride overflows size_t, in either region
        with pytest.raises(ce.Error) as e:
            ce.split_layout(d, p, [2 ** 62])
        assert e.value.code == ce.ERR_INVALID_ARGUMENT
    with pytest.raises(ce.Error) as e:
        ce.split_layout(3, 2, [2 ** 64 - 1])
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    with pytest.raises(ce.Error) as e:  # the sum of the parts overflows
        ce.split_layout(3, 2, [2 ** 61, 2 ** 61, 2 ** 61])
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    lib, out = ce._lib, ctypes.c_size_t(0)
    ok = (3, 2, _sz([5]), 1, _sz([0]), _sz([0]), ctypes.byref(out), ctypes.byref(out))
    assert lib.cec_split_layout(*ok) == ce.OK
    for i in (2, 4, 5, 6, 7):
        args = list(ok)
        args[i] = None
        assert lib.cec_split_layout(*args) == ce.ERR_INVALID_ARGUMENT, i


def test_encode_hash_split_argument_errors_in_order():
    rs = ce.ReedSolomon(3, 2)
    d, p = 3, 2
    lens = LENGTHS[:6]
    doffs, poffs, db, pb = ce.split_layout(d, p, lens)
    # 1. null pointers, even beside every later error
    for null in ("codec", "data", "doffs", "parity", "poffs", "lens", "digests"):
        assert _split(rs, lens, doffs, poffs, null=(null,)) == ce.ERR_INVALID_ARGUMENT, null
        assert _split(rs, [0] * 6, doffs, poffs, dbase=BASE_D + 1, null=(null,)) == \
            ce.ERR_INVALID_ARGUMENT, null
    # 2. a zero chunk length, even beside a misaligned base and overlapping regions
    for k in range(len(lens)):
        bad = list(lens)
        bad[k] = 0
        assert _split(rs, bad, doffs, poffs) == ce.EMPTY_SHARD
        assert _split(rs, bad, doffs, poffs, dbase=BASE_D + 1) == ce.EMPTY_SHARD
        assert _split(rs, bad, doffs, poffs, pbase=BASE_D) == ce.EMPTY_SHARD
    # 3. a base or an offset that is not a multiple of 16
    for delta in (1, 8, 15):
        assert _split(rs, lens, doffs, poffs, dbase=BASE_D + delta) == ce.ERR_INVALID_ARGUMENT
        assert _split(rs, lens, doffs, poffs, pbase=BASE_P + delta) == ce.ERR_INVALID_ARGUMENT
        for k in range(len(lens)):
            bad = list(doffs)
            bad[k] += delta
            assert _split(rs, lens, bad, poffs) == ce.ERR_INVALID_ARGUMENT
            bad = list(poffs)
            bad[k] += delta
            assert _split(rs, lens, doffs, bad) == ce.ERR_INVALID_ARGUMENT
    #    offsets not ascending and disjoint within a region
    for k in range(1, len(lens)):
        bad = list(doffs)
        bad[k] -= 16
        assert _split(rs, lens, bad, poffs) == ce.ERR_INVALID_ARGUMENT, k
        bad = list(poffs)
        bad[k] -= 16
        assert _split(rs, lens, doffs, bad) == ce.ERR_INVALID_ARGUMENT, k
    assert _split(rs, [16, 16], [0, 0], [0, 32]) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, [16, 16], [0, 48], [32, 0]) == ce.ERR_INVALID_ARGUMENT
    #    the two regions' byte ranges overlapping: the same place, one byte range into the other
    #    from either side, one region inside the other's spaced offsets
    assert _split(rs, lens, doffs, poffs, pbase=BASE_D) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, lens, doffs, poffs, pbase=BASE_D + db - 16) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, lens, doffs, poffs, pbase=BASE_D - pb + 16) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, [16, 16], [0, 4096], [0, 32], pbase=BASE_D + 1024) == \
        ce.ERR_INVALID_ARGUMENT
    #    counts beyond the kernels' 32-bit indices, a part that overflows, too many work units
    assert _split(rs, [16], [0], [0], n=(1 << 32) // 5 + 1) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, [2 ** 62], [0], [0]) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, [2 ** 64 - 1], [0], [0]) == ce.ERR_INVALID_ARGUMENT
    assert _split(rs, [1 << 50], [0], [0], dbase=1 << 60) == ce.ERR_INVALID_ARGUMENT
    # 4. sound arguments (touching regions, spaced offsets, parity below or above): no device
    if ce.device_count() == 0:
        spaced_d = [o + 4096 * k for k, o in enumerate(doffs)]
        spaced_p = [o + 256 * k for k, o in enumerate(poffs)]
        assert _split(rs, lens, doffs, poffs) == ce.ERR_NO_DEVICE
        assert _split(rs, lens, spaced_d, spaced_p) == ce.ERR_NO_DEVICE
        assert _split(rs, lens, doffs, poffs, pbase=BASE_D + db) == ce.ERR_NO_DEVICE
        assert _split(rs, lens, doffs, poffs, pbase=BASE_D - pb) == ce.ERR_NO_DEVICE


def test_split_zero_parts_is_ok():
    rs = ce.ReedSolomon(3, 2)
    assert ce._lib.cec_encode_hash_split(rs.handle, None, None, None, None, None, 0, None,
                                         None) == ce.OK
    ce.encode_hash_split(rs, 0, [], 0, [], [], 0)
    with pytest.raises(ValueError):
        ce.encode_hash_split(rs, 0, [0], 0, [], [16], 0)


def test_parts_pipeline_new_errors_in_order():
    rs = ce.ReedSolomon(3, 2)
    lib = ce._lib
    out = ce._vp()
    new = lib.cec_parts_pipeline_new
    assert new(None, 1 << 20, 64, 2, ctypes.byref(out)) == ce.ERR_INVALID_ARGUMENT
    assert new(rs.handle, 1 << 20, 64, 2, None) == ce.ERR_INVALID_ARGUMENT
    # the shape, before the device is looked for
    for slot_bytes, max_parts, depth in ((1 << 20, 64, 0), (1 << 20, 0, 2), (3 * 16 - 1, 64, 2),
                                         (0, 64, 2), (2 ** 64 - 1, 64, 2), (1 << 20, 2 ** 60, 2),
                                         (1 << 20, (1 << 32) // 5 + 1, 2)):
        assert new(rs.handle, slot_bytes, max_parts, depth, ctypes.byref(out)) == \
            ce.ERR_INVALID_ARGUMENT, (slot_bytes, max_parts, depth)
        assert not out
    assert b"slot_data_bytes" in lib.cec_last_error()
    with pytest.raises(ce.Error) as e:
        ce.PartsPipeline(rs, 1 << 20, 64, 0)
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    if ce.device_count() == 0:
        assert new(rs.handle, 3 * 16, 1, 1, ctypes.byref(out)) == ce.ERR_NO_DEVICE
        assert new(rs.handle, 1 << 20, 64, 2, ctypes.byref(out)) == ce.ERR_NO_DEVICE
        with pytest.raises(ce.Error) as e:
            ce.PartsPipeline(rs, 1 << 20, 64, 2)
        assert e.value.code == ce.ERR_NO_DEVICE


def test_parts_pipeline_calls_refuse_a_null_pipeline():
    lib = ce._lib
    slot, ptr, n = ctypes.c_size_t(0), ce._u8p(), ctypes.c_size_t(0)
    bufs = (ce._u8p * 1)()
    assert lib.cec_parts_pipeline_depth(None) == 0
    assert lib.cec_parts_pipeline_acquire(None, ctypes.byref(slot), ctypes.byref(ptr)) == \
        ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_pipeline_submit(None, 0, _sz([16]), 1) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_pipeline_submit(None, 0, _sz([0]), 1) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_pipeline_submit_from(None, 0, bufs, _sz([0]), 1, _sz([0])) == \
        ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_pipeline_wait(None, 0, ctypes.byref(ptr), ctypes.byref(ptr),
                                       ctypes.byref(n)) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_pipeline_query(None, 0) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_pipeline_drain(None) == ce.ERR_INVALID_ARGUMENT
    lib.cec_parts_pipeline_free(None)
