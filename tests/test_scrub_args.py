"""The segmented scrub, the part that needs no GPU: every argument check of cec_verify_segments and
cec_scrub_pipeline_new comes before any device use and in the order the header states, each beside
every later error, with device pointers that are never dereferenced; and the pipeline's calls
refuse a null handle.  (The refusals of cec_scrub_pipeline_submit_from need a pipeline, which needs
a device: their rule table is segment_words.hpp's, run on the CPU by tests/test_segment_words.py,
and the call itself runs in tests/test_gpu_scrub_pipeline.py.)"""
import ctypes

import pytest

import chunky_ec as ce

BASE, POOL, EXP, OK = 1 << 30, 1 << 40, 1 << 41, (1 << 42) + 3  # never dereferenced
F, L, W = ce.SEG_FIRST, ce.SEG_LAST, ce.SEG_FIRST | ce.SEG_LAST
INV = ce.ERR_INVALID_ARGUMENT


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _ver(lens, flags, slots, n_slots=8, offs=None, base=BASE, pool=POOL, exp=EXP, ok=OK, n=None,
         null=()):
    """Raw cec_verify_segments over the packed layout of `lens`; `null` names the pointer
    arguments passed as NULL."""
    if offs is None:
        stride = [(x + 15) // 16 * 16 for x in lens]
        offs = [sum(stride[:k]) for k in range(len(lens))]
    m = max(len(lens), 1)
    return ce._lib.cec_verify_segments(
        None if "base" in null else base,
        None if "offs" in null else _sz(offs),
        None if "lens" in null else _sz(lens),
        len(lens) if n is None else n,
        None if "slots" in null else (ctypes.c_uint32 * m)(*slots),
        None if "flags" in null else (ctypes.c_uint8 * m)(*flags),
        None if "midstates" in null else pool,
        n_slots,
        None if "expected" in null else exp,
        None if "ok" in null else ok, None)


def test_verify_segments_argument_errors_in_order():
    lens, flags, slots = [64, 128, 100, 7], [F, 0, L, W], [0, 1, 2, 99]
    # 1. null pointers, even beside every later error (a zero length, a misaligned base, a length
    #    that is no multiple of 64, slots out of range and named twice)
    for null in ("base", "offs", "lens", "slots", "flags", "expected", "ok", "midstates"):
        assert _ver(lens, flags, slots, null=(null,)) == INV, null
        assert _ver([0, 65, 100, 7], [F, 0, L, W], [9, 9, 9, 9], base=BASE + 1,
                    null=(null,)) == INV, null
    #    no pool is needed when every entry is whole, whatever its slot
    if ce.device_count() == 0:
        assert _ver(lens, [W] * 4, slots, n_slots=0, null=("midstates",)) == ce.ERR_NO_DEVICE
    #    an entry count beyond the 32-bit item index is refused before the arrays are walked
    assert _ver([16], [W], [0], n=(1 << 32) + 1) == INV
    assert _ver([0], [0], [9], n=1 << 33, base=BASE + 1) == INV
    # 2. a zero length, even beside a misaligned base, a length that is no multiple of 64, a slot
    #    out of range and a slot named twice
    for k in range(4):
        bad = list(lens)
        bad[k] = 0
        assert _ver(bad, flags, slots) == ce.EMPTY_SHARD
        assert _ver(bad, flags, slots, base=BASE + 1) == ce.EMPTY_SHARD
        assert _ver(bad, flags, slots, exp=EXP + 8) == ce.EMPTY_SHARD
        assert _ver(bad, [0] * 4, [9, 9, 9, 9]) == ce.EMPTY_SHARD
    # 3. cec_verify_ragged's rules: alignment (of the base, the offsets, the pool and the expected
    #    rows), order, overlap, lengths within size_t; each beside the later errors too
    for delta in (1, 8, 15):
        for later in ((flags, slots), ([0] * 4, [9, 9, 9, 9])):
            assert _ver(lens, *later, base=BASE + delta) == INV
            assert _ver(lens, *later, pool=POOL + delta) == INV
            assert _ver(lens, *later, exp=EXP + delta) == INV
            assert _ver(lens, *later, offs=[0, 64 + delta, 256, 512]) == INV
    assert _ver([16, 16], [W, W], [0, 0], offs=[0, 0]) == INV      # overlap
    assert _ver([16, 16], [W, W], [0, 0], offs=[16, 0]) == INV     # order
    assert _ver([17, 16], [W, W], [0, 0], offs=[0, 16]) == INV     # inside the stride
    assert _ver([2 ** 64 - 8], [W], [0]) == INV
    assert _ver([1 << 62], [W], [0], offs=[2 ** 64 - 16]) == INV
    #    ok is a byte array: any alignment
    # 4. an entry that is not LAST with a length that is no multiple of 64, even beside 5 and 6
    for fl in (F, 0):
        for bad_len in (1, 63, 65, 100):
            assert _ver([64, bad_len], [F, fl], [0, 1]) == INV
            assert b"multiple of 64" in ce._lib.cec_last_error()
            assert _ver([64, bad_len], [F, fl], [9, 9]) == INV
            assert b"multiple of 64" in ce._lib.cec_last_error()
    # 5. a slot >= n_state_slots, even beside 6
    assert _ver(lens, flags, [0, 8, 2, 99]) == INV
    assert b"n_state_slots" in ce._lib.cec_last_error()
    assert _ver(lens, flags, [8, 8, 2, 99]) == INV
    assert b"n_state_slots" in ce._lib.cec_last_error()
    assert _ver(lens, flags, slots, n_slots=2) == INV
    assert _ver(lens, flags, slots, n_slots=0) == INV
    # 6. a slot named by two record-touching entries
    for twice in ([0, 0, 2, 99], [0, 1, 1, 99], [2, 1, 2, 2]):
        assert _ver(lens, flags, twice) == INV
        assert b"same state slot" in ce._lib.cec_last_error()
    # 7. sound arguments: no device.  A whole entry's slot may be anything, also another's.
    if ce.device_count() == 0:
        assert _ver(lens, flags, slots) == ce.ERR_NO_DEVICE
        assert _ver(lens, flags, [0, 1, 2, 1]) == ce.ERR_NO_DEVICE
        assert _ver(lens, [F, 0, L, W], [7, 6, 5, 7]) == ce.ERR_NO_DEVICE
        assert _ver(lens, flags, slots, offs=[0, 64, 256, 1024]) == ce.ERR_NO_DEVICE  # gaps
        with pytest.raises(ce.Error) as e:
            ce.verify_segments(BASE, [0], [64], [0], [F], POOL, 1, EXP, OK)
        assert e.value.code == ce.ERR_NO_DEVICE


def test_zero_segments_is_ok():
    assert ce._lib.cec_verify_segments(None, None, None, 0, None, None, None, 0, None, None,
                                       None) == ce.OK
    ce.verify_segments(0, [], [], [], [], 0, 0, 0, 0)


def test_scrub_pipeline_new_errors_in_order():
    out = ce._vp()
    new = ce._lib.cec_scrub_pipeline_new
    assert new(1 << 20, 64, 2, 4, None) == INV
    assert new(1 << 20, 0, 0, 2 ** 62, None) == INV  # beside every later error
    # the size rules, before the device is looked for, each also beside a pool that is too large
    for slot_bytes, max_entries, depth in ((1 << 20, 64, 0), (1 << 20, 64, 17), (1 << 20, 0, 2),
                                           (15, 64, 2), (0, 64, 2), (2 ** 64 - 1, 64, 2),
                                           (2 ** 64 - 64, 64, 2), (1 << 20, 1 << 32, 2),
                                           (1 << 20, 2 ** 64 - 1, 2)):
        for max_open in (4, 2 ** 62):
            assert new(slot_bytes, max_entries, depth, max_open, ctypes.byref(out)) == INV
            assert not out
            assert b"cec_scrub_pipeline_new: depth" in ce._lib.cec_last_error()
    # a pool beyond the kernel's 32-bit record index
    for max_open in (1 << 32, 2 ** 62, 2 ** 64 - 1):
        assert new(1 << 20, 64, 2, max_open, ctypes.byref(out)) == INV
        assert b"max_open" in ce._lib.cec_last_error()
    with pytest.raises(ce.Error) as e:
        ce.ScrubPipeline(1 << 20, 64, 0, 4)
    assert e.value.code == INV
    if ce.device_count() == 0:
        for max_open in (0, 4):
            assert new(1 << 20, 64, 2, max_open, ctypes.byref(out)) == ce.ERR_NO_DEVICE
        with pytest.raises(ce.Error) as e:
            ce.ScrubPipeline(1 << 20, 64, 2, 4)
        assert e.value.code == ce.ERR_NO_DEVICE


def test_scrub_pipeline_calls_refuse_a_null_pipeline():
    lib = ce._lib
    slot, ptr, n = ctypes.c_size_t(0), ce._u8p(), ctypes.c_size_t(0)
    bufs = (ce._u8p * 1)()
    ids = (ctypes.c_uint32 * 1)()
    exp = (ctypes.c_uint8 * 32)()
    assert lib.cec_scrub_pipeline_depth(None) == 0
    assert lib.cec_scrub_pipeline_open_count(None) == 0
    assert lib.cec_scrub_pipeline_acquire(None, ctypes.byref(slot)) == INV
    assert lib.cec_scrub_pipeline_submit_from(None, 0, bufs, _sz([0]), _sz([0]), _sz([0]), ids,
                                              exp, 1) == INV
    assert lib.cec_scrub_pipeline_submit_from(None, 0, None, None, None, None, None, None,
                                              0) == INV
    assert lib.cec_scrub_pipeline_wait(None, 0, ctypes.byref(ptr), ctypes.byref(n)) == INV
    assert lib.cec_scrub_pipeline_query(None, 0) == INV
    assert lib.cec_scrub_pipeline_drain(None) == INV
    assert lib.cec_scrub_pipeline_abandon(None, 0) == INV
    lib.cec_scrub_pipeline_free(None)
