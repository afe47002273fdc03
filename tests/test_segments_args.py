"""Segmented ragged writes, the part that needs no GPU: every argument check of
cec_encode_hash_segments and cec_segment_pipeline_new comes before any device use and in the order
the header states, and the pipeline's calls refuse a null handle.  (The refusals of
cec_segment_pipeline_submit_from need a pipeline, which needs a device: their rule table runs on
the CPU in tests/test_segment_words.py and the call itself in tests/test_gpu_segment_pipeline.py.)"""
import ctypes

import pytest

import chunky_ec as ce

BASE_D, BASE_P, POOL = 1 << 30, 1 << 20, 1 << 40  # never dereferenced
F, L, W = ce.SEG_FIRST, ce.SEG_LAST, ce.SEG_FIRST | ce.SEG_LAST
INV = ce.ERR_INVALID_ARGUMENT


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _seg(rs, lens, flags, slots, n_slots=8, doffs=None, poffs=None, dbase=BASE_D, pbase=BASE_P,
         pool=POOL, n=None, null=()):
    """Raw cec_encode_hash_segments over the packed split layout of `lens`; `null` names the
    pointer arguments passed as NULL."""
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    if doffs is None:
        stride = [(x + 15) // 16 * 16 for x in lens]
        doffs = [d * sum(stride[:k]) for k in range(len(lens))]
        poffs = [p * sum(stride[:k]) for k in range(len(lens))]
    m = max(len(lens), 1)
    return ce._lib.cec_encode_hash_segments(
        None if "codec" in null else rs.handle,
        None if "data" in null else dbase,
        None if "doffs" in null else _sz(doffs),
        None if "parity" in null else pbase,
        None if "poffs" in null else _sz(poffs),
        None if "lens" in null else _sz(lens),
        len(lens) if n is None else n,
        None if "slots" in null else (ctypes.c_uint32 * m)(*slots),
        None if "flags" in null else (ctypes.c_uint8 * m)(*flags),
        None if "midstates" in null else pool,
        n_slots,
        None if "digests" in null else 16, None)


def test_midstate_record_is_48_bytes():
    assert ce._lib.cec_sha_midstate_bytes() == 48 == ce.MIDSTATE_BYTES
    assert (ce.SEG_FIRST, ce.SEG_LAST) == (1, 2)


def test_encode_hash_segments_argument_errors_in_order():
    rs = ce.ReedSolomon(3, 2)
    lens, flags, slots = [64, 128, 100, 7], [F, 0, L, W], [0, 1, 2, 99]
    # 1. null pointers, even beside every later error
    for null in ("codec", "data", "doffs", "parity", "poffs", "lens", "slots", "flags", "digests",
                 "midstates"):
        assert _seg(rs, lens, flags, slots, null=(null,)) == INV, null
        assert _seg(rs, [0, 65, 100, 7], [F, 0, L, W], [9, 9, 9, 9], dbase=BASE_D + 1,
                    null=(null,)) == INV, null
    #    no pool is needed when every entry is a whole part, whatever its slot
    if ce.device_count() == 0:
        assert _seg(rs, lens, [W] * 4, slots, n_slots=0, null=("midstates",)) == ce.ERR_NO_DEVICE
    # 2. a zero length, even beside a misaligned base, a length that is no multiple of 64, a slot
    #    out of range and a slot named twice
    for k in range(4):
        bad = list(lens)
        bad[k] = 0
        assert _seg(rs, bad, flags, slots) == ce.EMPTY_SHARD
        assert _seg(rs, bad, flags, slots, dbase=BASE_D + 1) == ce.EMPTY_SHARD
        assert _seg(rs, bad, [0] * 4, [9, 9, 9, 9]) == ce.EMPTY_SHARD
    # 3. cec_encode_hash_split's rules: alignment, order, overlap, the counts
    for delta in (1, 8, 15):
        assert _seg(rs, lens, flags, slots, dbase=BASE_D + delta) == INV
        assert _seg(rs, lens, flags, slots, pbase=BASE_P + delta) == INV
        assert _seg(rs, lens, flags, slots, pool=POOL + delta) == INV
    assert _seg(rs, [16, 16], [W, W], [0, 0], doffs=[0, 0], poffs=[0, 32]) == INV
    assert _seg(rs, [16, 16], [W, W], [0, 0], doffs=[0, 48], poffs=[32, 0]) == INV
    assert _seg(rs, lens, flags, slots, pbase=BASE_D) == INV
    assert b"overlap" in ce._lib.cec_last_error()
    assert _seg(rs, [16], [W], [0], n=(1 << 32) // 5 + 1) == INV
    assert _seg(rs, [2 ** 62], [W], [0]) == INV
    # 4. an entry that is not LAST with a length that is no multiple of 64, even beside 5 and 6
    for fl in (F, 0):
        for bad_len in (1, 63, 65, 100):
            assert _seg(rs, [64, bad_len], [F, fl], [0, 1]) == INV
            assert b"multiple of 64" in ce._lib.cec_last_error()
            assert _seg(rs, [64, bad_len], [F, fl], [9, 9]) == INV
            assert b"multiple of 64" in ce._lib.cec_last_error()
    # 5. a slot >= n_state_slots, even beside 6
    assert _seg(rs, lens, flags, [0, 8, 2, 99]) == INV
    assert b"n_state_slots" in ce._lib.cec_last_error()
    assert _seg(rs, lens, flags, [8, 8, 2, 99]) == INV
    assert b"n_state_slots" in ce._lib.cec_last_error()
    assert _seg(rs, lens, flags, slots, n_slots=2) == INV
    assert _seg(rs, lens, flags, slots, n_slots=0) == INV
    # 6. a slot named by two record-touching entries
    for twice in ([0, 0, 2, 99], [0, 1, 1, 99], [2, 1, 2, 2]):
        assert _seg(rs, lens, flags, twice) == INV
        assert b"same state slot" in ce._lib.cec_last_error()
    # 7. sound arguments: no device.  A whole part's slot may be anything, also another's.
    if ce.device_count() == 0:
        assert _seg(rs, lens, flags, slots) == ce.ERR_NO_DEVICE
        assert _seg(rs, lens, flags, [0, 1, 2, 1]) == ce.ERR_NO_DEVICE
        assert _seg(rs, lens, [F, 0, L, W], [7, 6, 5, 7]) == ce.ERR_NO_DEVICE
        with pytest.raises(ce.Error) as e:
            ce.encode_hash_segments(rs, BASE_D, [0], BASE_P, [0], [64], [0], [F], POOL, 1, 16)
        assert e.value.code == ce.ERR_NO_DEVICE


def test_zero_segments_is_ok():
    rs = ce.ReedSolomon(3, 2)
    assert ce._lib.cec_encode_hash_segments(rs.handle, None, None, None, None, None, 0, None, None,
                                            None, 0, None, None) == ce.OK
    ce.encode_hash_segments(rs, 0, [], 0, [], [], [], [], 0, 0, 0)
    assert ce._lib.cec_encode_hash_segments(None, None, None, None, None, None, 0, None, None,
                                            None, 0, None, None) == INV


def test_segment_pipeline_new_errors_in_order():
    rs = ce.ReedSolomon(3, 2)
    out = ce._vp()
    new = ce._lib.cec_segment_pipeline_new
    assert new(None, 1 << 20, 64, 2, 4, ctypes.byref(out)) == INV
    assert new(rs.handle, 1 << 20, 64, 2, 4, None) == INV
    # the parts pipeline's shape rules, before the device is looked for
    for slot_bytes, max_parts, depth in ((1 << 20, 64, 0), (1 << 20, 64, 17), (1 << 20, 0, 2),
                                         (3 * 16 - 1, 64, 2), (2 ** 64 - 1, 64, 2),
                                         (1 << 20, (1 << 32) // 5 + 1, 2)):
        assert new(rs.handle, slot_bytes, max_parts, depth, 4, ctypes.byref(out)) == INV
        assert not out
        assert b"cec_segment_pipeline_new" in ce._lib.cec_last_error()
    # a pool beyond the kernel's 32-bit record index
    for max_open in ((1 << 32) // 5 + 1, 2 ** 62):
        assert new(rs.handle, 1 << 20, 64, 2, max_open, ctypes.byref(out)) == INV
        assert b"max_open" in ce._lib.cec_last_error()
    with pytest.raises(ce.Error) as e:
        ce.SegmentPipeline(rs, 1 << 20, 64, 0, 4)
    assert e.value.code == INV
    if ce.device_count() == 0:
        for max_open in (0, 4):
            assert new(rs.handle, 1 << 20, 64, 2, max_open, ctypes.byref(out)) == ce.ERR_NO_DEVICE
        with pytest.raises(ce.Error) as e:
            ce.SegmentPipeline(rs, 1 << 20, 64, 2, 4)
        assert e.value.code == ce.ERR_NO_DEVICE


def test_segment_pipeline_calls_refuse_a_null_pipeline():
    lib = ce._lib
    slot, ptr, n = ctypes.c_size_t(0), ce._u8p(), ctypes.c_size_t(0)
    bufs = (ce._u8p * 1)()
    ids = (ctypes.c_uint32 * 1)()
    assert lib.cec_segment_pipeline_depth(None) == 0
    assert lib.cec_segment_pipeline_open_count(None) == 0
    assert lib.cec_segment_pipeline_acquire(None, ctypes.byref(slot)) == INV
    assert lib.cec_segment_pipeline_submit_from(None, 0, bufs, _sz([0]), _sz([0]), _sz([0]), ids, 1,
                                                _sz([0])) == INV
    assert lib.cec_segment_pipeline_wait(None, 0, ctypes.byref(ptr), ctypes.byref(ptr),
                                         ctypes.byref(n)) == INV
    assert lib.cec_segment_pipeline_query(None, 0) == INV
    assert lib.cec_segment_pipeline_drain(None) == INV
    assert lib.cec_segment_pipeline_abandon(None, 0) == INV
    lib.cec_segment_pipeline_free(None)
