"""cec_part_encode's coalescer with calls of different chunk lengths in one batch
(CEC_COALESCE_MIXED=1): the batch is laid out in the split layout and run by the ragged encode's
launches, every caller still gets exactly its own part's parity and digests (against the CPU
oracle), and the counters show the sharing.  Integer work: every comparison is exact.

The chunk lengths are the column, 4 KiB-unit and pitch != stride edges, L in {1, 15, 16, 17, 4096,
4099, 65539}, and further lengths around them; every batch holds 64 KiB lengths, so a launch lasts
long enough for the other callers to queue behind it."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

EDGES = [1, 15, 16, 17, 4096, 4099, 65539]
# 48 distinct chunk lengths: the edges, 21 around 64 KiB and 20 between 4 KiB and 10 KiB
DISTINCT = EDGES + [65541 + 3 * i for i in range(21)] + [4100 + 257 * i for i in range(20)]
assert len(set(DISTINCT)) == len(DISTINCT) == 48
SHAPES = [(3, 2), (10, 4), (20, 8)]
CANARY, TAIL = 0xA5, 64
_ORACLE = {}


def _reference(d, p, L):
    """(data d*L bytes, parity (p, L), digests bytes) of the part of chunk length L: computed
    once, shared, never modified.  The part's last data chunk is short by one byte where that
    leaves the chunk length alone (the engine reads d*L bytes: the caller pads with zeros)."""
    key = (d, p, L)
    if key not in _ORACLE:
        length = d * L - (1 if L > 1 else 0)
        src = gen_bytes(7000 + 13 * L + d, length)
        cs, par, dig = oracle.part_encode(d, p, src, length)
        assert cs == L
        data = np.zeros(d * L, np.uint8)
        data[:length] = src
        _ORACLE[key] = (length, data, np.stack(par), b"".join(x.tobytes() for x in dig))
    return _ORACLE[key]


def _host(nbytes, pinned):
    arr = ce.HostBuffer(nbytes).array if pinned else np.empty(nbytes, np.uint8)
    assert ce.host_is_pinned(arr) == pinned
    return arr


def _encode_together(rs, lens, pins=None):
    """One cec_part_encode call per entry of `lens`, each on its own thread, all released by a
    barrier; pins[i] = (data page-locked, parity page-locked).  Every result against the oracle,
    the canary behind p*L of each parity buffer included.  Returns the counters' increments:
    (calls, launches, mixed batches)."""
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    n = len(lens)
    jobs = []
    for i, L in enumerate(lens):
        length, data, _, _ = _reference(d, p, L)
        in_pinned, out_pinned = pins[i] if pins else (False, False)
        src = _host(d * L, in_pinned)
        src[:] = data
        par = _host(p * L + TAIL, out_pinned)
        par[:] = CANARY
        jobs.append((length, src, par, (ctypes.c_uint8 * (32 * (d + p)))(), ctypes.c_size_t(0)))
    codes = [None] * n
    barrier = threading.Barrier(n)

    def call(i):
        length, src, par, dig, cs = jobs[i]
        barrier.wait()
        codes[i] = ce._lib.cec_part_encode(rs.handle, ctypes.cast(ce._addr(src), ce._u8p), length,
                                           ctypes.cast(ce._addr(par), ce._u8p), dig,
                                           ctypes.byref(cs))

    c0, l0 = ce.coalesce_stats()
    m0 = ce.coalesce_detail()[0]
    threads = [threading.Thread(target=call, args=(i,)) for i in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    c1, l1 = ce.coalesce_stats()
    m1 = ce.coalesce_detail()[0]
    assert codes == [ce.OK] * n, codes
    for i, L in enumerate(lens):
        _, _, ref_par, ref_dig = _reference(d, p, L)
        _, _, par, dig, cs = jobs[i]
        assert cs.value == L, i
        assert np.array_equal(par[:p * L].reshape(p, L), ref_par), (i, L, "parity")
        assert np.all(par[p * L:] == CANARY), (i, L, "bytes behind the parity")
        assert bytes(dig) == ref_dig, (i, L, "digests")
    return c1 - c0, l1 - l0, m1 - m0


@pytest.mark.parametrize("d,p", SHAPES)
def test_calls_of_distinct_lengths_share_launches(d, p, knob_env):
    knob_env.set("CEC_COALESCE_MIXED", "1")
    calls, launches, mixed = _encode_together(ce.ReedSolomon(d, p), DISTINCT)
    print(f"RS({d},{p}): {calls} calls, {launches} launches, {mixed} mixed batches")
    assert calls == 48 and launches < 48
    assert mixed >= 1


def test_knob_at_zero_gathers_by_length(knob_env):
    knob_env.set("CEC_COALESCE_MIXED", "0")
    calls, launches, mixed = _encode_together(ce.ReedSolomon(3, 2), DISTINCT)
    assert calls == 48 and launches == 48 and mixed == 0


def test_uniform_batch_under_the_knob_takes_the_strided_path(knob_env):
    knob_env.set("CEC_COALESCE_MIXED", "1")
    calls, launches, mixed = _encode_together(ce.ReedSolomon(10, 4), [65539] * 48)
    assert calls == 48 and launches < 48 and mixed == 0


def test_page_locked_and_pageable_callers_in_one_mixed_batch(knob_env):
    """Page-locked x pageable x in / out, at chunk lengths that are their own 16-byte stride (the
    1-D copies) and that are not (the 2-D copies), beside staged parts."""
    knob_env.set("CEC_COALESCE_MIXED", "1")
    lens = [16, 32, 4096, 8192, 65536, 65552, 1, 15, 17, 4099, 65539, 65541]
    assert sum(L % 16 == 0 for L in lens) == 6
    combos = [(True, True), (True, False), (False, True), (False, False)]
    for d, p in [(3, 2), (10, 4)]:
        calls, launches, mixed = _encode_together(
            ce.ReedSolomon(d, p), [L for L in lens for _ in combos], [c for _ in lens for c in combos])
        assert calls == 48 and launches < 48 and mixed >= 1


def test_mixed_batch_through_the_fused_ragged_kernel(knob_env):
    knob_env.set("CEC_COALESCE_MIXED", "1")
    knob_env.set("CEC_RAGGED_FUSED", "1")
    f0, _ = ce.ragged_stats()
    calls, launches, mixed = _encode_together(ce.ReedSolomon(10, 4), DISTINCT)
    f1, _ = ce.ragged_stats()
    assert calls == 48 and launches < 48 and mixed >= 1
    assert f1 - f0 >= 1


def test_small_cap_splits_the_callers_into_several_batches(knob_env):
    knob_env.set("CEC_COALESCE_MIXED", "1")
    knob_env.set("CEC_COALESCE_MAX_MIB", "1")
    calls, launches, mixed = _encode_together(ce.ReedSolomon(10, 4), DISTINCT)
    # 22 parts of about 640 KiB of data each: no two of them fit one batch
    assert calls == 48 and launches >= 22
