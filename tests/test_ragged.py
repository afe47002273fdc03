"""Ragged batches, the part that needs no GPU: the layout functions and every argument check of
cec_encode_hash_ragged / cec_parts_encode, which all come before any device use."""
import ctypes

import pytest

import chunky_ec as ce

LENS = [1, 15, 16, 17, 683]


def _sz(values):
    return (ctypes.c_size_t * max(len(values), 1))(*values)


def _ragged(rs, base, offs, lens, n=None, digests=16, null=()):
    """Raw cec_encode_hash_ragged; `null` names the pointer arguments passed as NULL."""
    a_offs, a_lens = _sz(offs), _sz(lens)
    return ce._lib.cec_encode_hash_ragged(
        None if "codec" in null else rs.handle,
        None if "base" in null else base,
        None if "offs" in null else a_offs,
        None if "lens" in null else a_lens,
        len(lens) if n is None else n,
        None if "digests" in null else digests, None)


def test_ragged_stride_values():
    assert [ce.ragged_stride(x) for x in LENS] == [16, 16, 16, 32, 688]
    assert ce.ragged_stride(0) == 0
    assert ce.ragged_stride(1 << 20) == 1 << 20
    assert ce.ragged_stride((1 << 20) + 1) == (1 << 20) + 16
    assert ce.ragged_stride(2 ** 64 - 1) == 0  # would overflow: no stride


@pytest.mark.parametrize("t", [2, 5, 14, 28])
def test_ragged_layout_values(t):
    offs, total = ce.ragged_layout(t, LENS)
    strides = [(x + 15) // 16 * 16 for x in LENS]
    want, at = [], 0
    for s in strides:
        want.append(at)
        at += t * s
    assert offs == want and total == at
    assert all(o % 16 == 0 for o in offs)
    assert all(b > a for a, b in zip(offs, offs[1:]))
    # parts are disjoint: the next one starts at or behind the end of this one's last chunk
    for k in range(len(LENS) - 1):
        assert offs[k + 1] >= offs[k] + t * strides[k]
    assert ce.ragged_layout(t, []) == ([], 0)


def test_ragged_layout_errors():
    for lens in ([0], [5, 0, 5]):
        with pytest.raises(ce.Error) as e:
            ce.ragged_layout(5, lens)
        assert e.value.code == ce.EMPTY_SHARD
    with pytest.raises(ce.Error) as e:
        ce.ragged_layout(0, [5])
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    with pytest.raises(ce.Error) as e:
        ce.ragged_layout(5, [2 ** 62])  # 5 * stride overflows size_t
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    total = ctypes.c_size_t(0)
    lib = ce._lib
    assert lib.cec_ragged_layout(5, None, 1, _sz([0]), ctypes.byref(total)) == \
        ce.ERR_INVALID_ARGUMENT
    assert lib.cec_ragged_layout(5, _sz([5]), 1, None, ctypes.byref(total)) == \
        ce.ERR_INVALID_ARGUMENT
    assert lib.cec_ragged_layout(5, _sz([5]), 1, _sz([0]), None) == ce.ERR_INVALID_ARGUMENT


def test_encode_hash_ragged_argument_errors_precede_device_use():
    rs = ce.ReedSolomon(3, 2)
    t = 5
    offs, total = ce.ragged_layout(t, LENS)
    base = 1 << 20  # never dereferenced: every case below returns before any device use
    for null in ("codec", "base", "offs", "lens", "digests"):
        assert _ragged(rs, base, offs, LENS, null=(null,)) == ce.ERR_INVALID_ARGUMENT, null
    # a zero chunk length anywhere: EmptyShard, nothing launched
    for k in range(len(LENS)):
        lens = list(LENS)
        lens[k] = 0
        assert _ragged(rs, base, offs, lens) == ce.EMPTY_SHARD
    # base or an offset not a multiple of 16
    for b in (base + 1, base + 8, base + 15):
        assert _ragged(rs, b, offs, LENS) == ce.ERR_INVALID_ARGUMENT
    for k in range(len(LENS)):
        for delta in (1, 8, 15):
            bad = list(offs)
            bad[k] += delta
            assert _ragged(rs, base, bad, LENS) == ce.ERR_INVALID_ARGUMENT
    # parts not ascending and disjoint: off[k+1] < off[k] + (d+p) * stride(L_k)
    for k in range(1, len(LENS)):
        bad = list(offs)
        bad[k] -= 16
        assert _ragged(rs, base, bad, LENS) == ce.ERR_INVALID_ARGUMENT, k
    assert _ragged(rs, base, [offs[1], offs[0]], LENS[:2]) == ce.ERR_INVALID_ARGUMENT
    assert _ragged(rs, base, [0, 0], [16, 16]) == ce.ERR_INVALID_ARGUMENT
    # counts beyond the kernels' 32-bit indices: more than 2^32 - 1 chunks (n_parts itself is
    # checked before the arrays are read), a part that overflows size_t, more work units than
    # one grid can hold
    assert _ragged(rs, base, [0], [16], n=(1 << 32) // t + 1) == ce.ERR_INVALID_ARGUMENT
    assert _ragged(rs, base, [0], [2 ** 62]) == ce.ERR_INVALID_ARGUMENT
    assert _ragged(rs, base, [0], [2 ** 64 - 1]) == ce.ERR_INVALID_ARGUMENT
    assert _ragged(rs, base, [0], [1 << 50]) == ce.ERR_INVALID_ARGUMENT
    # spaced (not packed) offsets are fine as far as the arguments go
    spaced = [o + 4096 * k for k, o in enumerate(offs)]
    if ce.device_count() == 0:
        assert _ragged(rs, base, spaced, LENS) == ce.ERR_NO_DEVICE
        assert _ragged(rs, base, offs, LENS) == ce.ERR_NO_DEVICE


def test_ragged_zero_parts_is_ok():
    rs = ce.ReedSolomon(3, 2)
    assert _ragged(rs, 1 << 20, [], [], n=0) == ce.OK
    assert ce._lib.cec_encode_hash_ragged(rs.handle, None, None, None, 0, None, None) == ce.OK
    ce.encode_hash_ragged(rs, 0, [], [], 0)
    assert ce._lib.cec_parts_encode(rs.handle, None, None, 0, None, None, None) == ce.OK
    assert ce.parts_encode(rs, []) == []


def _parts_encode_raw(rs, bufs, null=()):
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    n = len(bufs)
    keep = []
    ptrs = (ce._u8p * n)(*[ce._buf_ptr(b, keep) for b in bufs])
    lens = _sz([len(b) for b in bufs])
    pars = [(ctypes.c_uint8 * max(p * ((len(b) + d - 1) // d), 1))() for b in bufs]
    par_ptrs = (ce._u8p * n)(*[ctypes.cast(x, ce._u8p) for x in pars])
    dig = (ctypes.c_uint8 * (32 * (d + p) * n))()
    ctypes.memset(dig, 0xEE, len(dig))
    for x in pars:
        ctypes.memset(x, 0xEE, len(x))
    cs = (ctypes.c_size_t * n)(*([77] * n))
    code = ce._lib.cec_parts_encode(
        None if "codec" in null else rs.handle,
        None if "bufs" in null else ptrs,
        None if "lens" in null else lens, n,
        None if "parity" in null else par_ptrs,
        None if "digests" in null else dig,
        None if "chunksizes" in null else cs)
    untouched = (all(b == 0xEE for b in bytes(dig)) and
                 all(b == 0xEE for x in pars for b in bytes(x)) and list(cs) == [77] * n)
    return code, untouched


def test_parts_encode_argument_errors_precede_device_use():
    rs = ce.ReedSolomon(3, 2)
    bufs = [b"a" * 7, b"b" * 20480, b"c"]
    for null in ("codec", "bufs", "lens", "parity", "digests", "chunksizes"):
        code, untouched = _parts_encode_raw(rs, bufs, null=(null,))
        assert code == ce.ERR_INVALID_ARGUMENT and untouched, null
    # a zero length anywhere in the list: EmptyShard before anything is written
    for k in range(3):
        bad = list(bufs)
        bad[k] = b""
        code, untouched = _parts_encode_raw(rs, bad)
        assert code == ce.EMPTY_SHARD and untouched, k
        with pytest.raises(ce.Error) as e:
            ce.parts_encode(rs, bad)
        assert e.value.code == ce.EMPTY_SHARD
    if ce.device_count() == 0:
        code, untouched = _parts_encode_raw(rs, bufs)
        assert code == ce.ERR_NO_DEVICE and untouched
