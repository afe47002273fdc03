"""The ragged read pipeline on the GPU (cec_parts_reader_*): batches of parts of different chunk
lengths through slots in flight, only the rebuilt chunks coming back, packed; against
cec_parts_read on the same inputs and the CPU oracle's original chunks.  Integer work: every
comparison is exact."""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import LENGTHS, _stride  # noqa: E402
from test_gpu_ragged_read import VERIFIED, _oracle_parts  # noqa: E402

SHAPES = [(3, 2), (10, 4)]
SLOT, MAX_PARTS, DEPTH, BATCHES = 1 << 20, 64, 2, 7
MODES = pytest.mark.parametrize("data_only", [True, False], ids=["data_only", "all"])


@pytest.fixture(scope="module")
def reference():
    """Per shape and batch, one oracle part (chunks (d+p, L), digests) per chunk length of
    LENGTHS[b::BATCHES]: computed once, shared, never modified."""
    return {(d, p): [_oracle_parts(d, p, LENGTHS[b::BATCHES], 100 * d + 10 * p + b)
                     for b in range(BATCHES)] for d, p in SHAPES}


def _batch(d, p, oracle_parts, b, flip=()):
    """parts_read's arguments for a batch: part q misses (q + b) % (p + 1) chunks at seeded
    places, a data chunk among them whenever it misses any, and has one loaded chunk flagged
    PRESENT_VERIFIED when q % 3 == 2; `flip` lists (q, i) whose first byte is loaded flipped.
    Returns (parts, expected)."""
    t = d + p
    rng = np.random.default_rng(1000 * d + 10 * b)
    parts, expected = [], []
    for q, (chunks, dig) in enumerate(oracle_parts):
        order = rng.permutation(t).tolist()
        order.insert(0, order.pop(next(x for x, i in enumerate(order) if i < d)))
        gone = set(order[:(q + b) % (p + 1)])
        row = []
        for i in range(t):
            if i in gone:
                row.append(None)
                continue
            c = chunks[i].copy()
            if (q, i) in flip:
                c[0] ^= 0x01
            row.append(c.tobytes())
        if q % 3 == 2:
            i = next(i for i in range(t) if row[i] is not None and (q, i) not in flip)
            row[i] = (row[i], VERIFIED)
        parts.append(row)
        expected.append([dig[i].tobytes() for i in range(t)])
    return parts, expected


def _lens(parts):
    return [len(next(c[0] if isinstance(c, tuple) else c for c in row if c is not None))
            for row in parts]


def _check_original(d, data_only, oracle_parts, got):
    """Every part decodes, and every slot of the mode holds the oracle's chunk."""
    chunks, verified, status = got
    assert status == [ce.OK] * len(oracle_parts)
    for k, (orig, _) in enumerate(oracle_parts):
        for i in range(orig.shape[0]):
            if i < d or not data_only:
                c = chunks[k][i]
                assert bytes(c[0] if isinstance(c, tuple) else c) == orig[i].tobytes(), (k, i)


def _place(rd, stage, parts):
    """The caller's packing for submit: loaded chunks at the ragged layout's offsets, 0xA5 between
    and in the slots that are not loaded.  Returns (chunk_lens, flags)."""
    t = rd.d + rd.p
    lens = _lens(parts)
    offs, total = ce.ragged_layout(t, lens)
    stage[:total] = 0xA5
    flags = bytearray(len(parts) * t)
    for k, row in enumerate(parts):
        for i, c in enumerate(row):
            if c is None:
                continue
            data, flags[k * t + i] = (c[0], c[1]) if isinstance(c, tuple) else (c, 1)
            at = offs[k] + i * _stride(lens[k])
            stage[at:at + lens[k]] = np.frombuffer(data, np.uint8)
    return lens, bytes(flags)


def _unpack(rd, parts, lens, waited):
    """wait()'s views in parts_read's result form."""
    verified, status, rebuilt, offsets = waited
    d, t = rd.d, rd.d + rd.p
    assert verified.shape == (len(parts) * t,) and status.shape == (len(parts),)
    assert offsets.shape == (len(parts) + 1,) and rebuilt.shape == (int(offsets[-1]),)
    out = []
    for k, row in enumerate(parts):
        got, r = [], 0
        for i, c in enumerate(row):
            fillable = i < d or not rd.data_only
            if verified[k * t + i]:
                got.append(c[0] if isinstance(c, tuple) else c)
            elif status[k] == ce.OK and fillable:
                at = int(offsets[k]) + r * _stride(lens[k])
                got.append(rebuilt[at:at + lens[k]].tobytes())
                r += 1
            else:
                got.append(None)
        assert int(offsets[k + 1] - offsets[k]) == r * _stride(lens[k])
        out.append(got)
    return out, bytes(verified), [int(x) for x in status]


def _strip(result):
    chunks, verified, status = result
    return ([[bytes(c[0] if isinstance(c, tuple) else c) if c is not None else None for c in row]
             for row in chunks], verified, status)


def _stream(rd, batches, use_submit=False):
    """Every batch through the reader with all slots in flight, the oldest collected first."""
    pending, results, first = [], [], None

    def collect():
        slot, parts, lens = pending.pop(0)
        if use_submit:
            results.append(_strip(_unpack(rd, parts, lens, rd.wait(slot))))
        else:
            results.append(_strip(rd.collect(slot)))
    for b, (parts, expected) in enumerate(batches):
        if len(pending) == rd.depth:
            collect()
        slot, stage = rd.acquire()
        first = slot if first is None else first
        assert slot == (first + b) % rd.depth  # round-robin from wherever the reader stood
        assert stage.shape == (rd.slot_bytes,)
        if use_submit:
            lens, flags = _place(rd, stage, parts)
            rd.submit(slot, lens, flags, b"".join(h for row in expected for h in row))
        else:
            lens = _lens(parts)
            rd.submit_from(slot, parts, expected)
        pending.append((slot, parts, lens))
    while pending:
        collect()
    return results


@MODES
@pytest.mark.parametrize("d,p", SHAPES)
def test_seven_batches_equal_parts_read_and_the_original(d, p, data_only, reference):
    rs = ce.ReedSolomon(d, p)
    rd = ce.PartsReader(rs, SLOT, MAX_PARTS, DEPTH, data_only)
    assert rd.depth == DEPTH == ce._lib.cec_parts_reader_depth(rd._h)
    batches = [_batch(d, p, reference[(d, p)][b], b) for b in range(BATCHES)]
    results = _stream(rd, batches)  # 7 batches on 2 slots: each slot at least three times
    for b, ((parts, expected), got) in enumerate(zip(batches, results)):
        assert got == _strip(ce.parts_read(rs, parts, expected, data_only)), b
        _check_original(d, data_only, reference[(d, p)][b], got)


@MODES
@pytest.mark.parametrize("d,p", SHAPES)
def test_submit_equals_submit_from(d, p, data_only, reference):
    rd = ce.PartsReader(ce.ReedSolomon(d, p), SLOT, MAX_PARTS, DEPTH, data_only)
    batches = [_batch(d, p, reference[(d, p)][b], b, flip={(1, 0)} if b % 2 else ())
               for b in range(BATCHES)]
    assert _stream(rd, batches, use_submit=True) == _stream(rd, batches)


def test_scatter_fills_the_callers_slots_as_parts_read_does(reference):
    """Raw calls with the caller's own slot memory, 0xA5 where nothing is loaded: after scatter
    the slots equal cec_parts_read's byte for byte, the ones neither call may write included."""
    d, p = 3, 2
    t = d + p
    rs = ce.ReedSolomon(d, p)
    parts, expected = _batch(d, p, reference[(d, p)][3], 3, flip={(0, 1)})
    assert all(c is not None for c in parts[0])  # the flipped chunk has spares
    keep = next(i for i, c in enumerate(parts[1]) if c is not None)
    parts[1] = [c if i == keep else None for i, c in enumerate(parts[1])]  # cannot be decoded
    lens, n = _lens(parts), len(parts)
    flags = bytearray(n * t)
    exp = b"".join(h for row in expected for h in row)

    def slots():
        mem = []
        for k, row in enumerate(parts):
            for i, c in enumerate(row):
                buf = (ctypes.c_uint8 * lens[k])(*([0xA5] * lens[k]))
                if c is not None:
                    data, flags[k * t + i] = (c[0], c[1]) if isinstance(c, tuple) else (c, 1)
                    ctypes.memmove(buf, data, lens[k])
                mem.append(buf)
        return mem, (ce._u8p * (n * t))(*[ctypes.cast(m, ce._u8p) for m in mem])
    mem_a, ptr_a = slots()
    mem_b, ptr_b = slots()
    lens_c = (ctypes.c_size_t * n)(*lens)
    pres = (ctypes.c_uint8 * (n * t))(*flags)
    expc = (ctypes.c_uint8 * len(exp)).from_buffer_copy(exp)
    ver = (ctypes.c_uint8 * (n * t))()
    st = (ctypes.c_int * n)()
    assert ce._lib.cec_parts_read(rs.handle, ptr_a, lens_c, n, pres, expc, 1, ver, st) == ce.OK
    rd = ce.PartsReader(rs, SLOT, MAX_PARTS, 1, True)
    slot, _ = rd.acquire()
    assert ce._lib.cec_parts_reader_submit_from(rd._h, slot, ptr_b, lens_c, n, pres, expc) == ce.OK
    verified, status, _, _ = rd.wait(slot)
    assert bytes(verified) == bytes(ver) and list(status) == list(st)
    assert status[1] == ce.TOO_FEW_SHARDS_PRESENT and verified[0 * t + 1] == 0
    assert [bytes(m) for m in mem_b] != [bytes(m) for m in mem_a]  # not scattered yet
    assert ce._lib.cec_parts_reader_scatter(rd._h, slot, ptr_b) == ce.OK
    assert [bytes(m) for m in mem_b] == [bytes(m) for m in mem_a]
    # the NULL rule, before the first byte is copied: a slot the mode fills in a decodable part
    k = next(k for k in range(n) if status[k] == ce.OK and not all(verified[k * t:k * t + d]))
    i = next(i for i in range(d) if not verified[k * t + i])
    holes = list(ptr_b)
    holes[k * t + i] = ce._u8p()
    before = [bytes(m) for m in mem_b]
    assert ce._lib.cec_parts_reader_scatter(rd._h, slot, (ce._u8p * (n * t))(*holes)) == \
        ce.ERR_INVALID_ARGUMENT
    assert [bytes(m) for m in mem_b] == before
    assert ce._lib.cec_parts_reader_submit_from(rd._h, slot, (ce._u8p * (n * t))(*holes), lens_c, n,
                                                pres, expc) == ce.ERR_INVALID_ARGUMENT


def test_results_stay_until_the_slot_is_acquired_again(reference):
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    rd = ce.PartsReader(rs, SLOT, MAX_PARTS, DEPTH)
    b0, b3, b1 = (_batch(d, p, reference[(d, p)][b], b) for b in (0, 3, 1))
    s0, _ = rd.acquire()
    rd.submit_from(s0, *b0)
    views = rd.wait(s0)
    keep = [v.copy() for v in views]
    assert len(keep[2]) > 0
    s1, _ = rd.acquire()
    assert (s0, s1) == (0, 1)
    rd.submit_from(s1, *b3)
    assert _strip(rd.collect(s1)) == _strip(ce.parts_read(rs, *b3))
    # slot 0's views are still its batch, while and after slot 1 ran
    assert all(np.array_equal(v, k) for v, k in zip(views, keep))
    assert _strip(rd.collect(s0)) == _strip(ce.parts_read(rs, *b0))
    s2, _ = rd.acquire()
    assert s2 == 0
    rd.submit_from(s2, *b1)
    assert _strip(rd.collect(s2)) == _strip(ce.parts_read(rs, *b1))
    assert not np.array_equal(views[2][:16], keep[2][:16])  # gone: the new batch's


@pytest.mark.parametrize("d,p", SHAPES)
def test_slot_capacity_and_refused_batches(d, p, reference):
    t = d + p
    rs = ce.ReedSolomon(d, p)
    L = 4097
    (chunks, dig), = _oracle_parts(d, p, [L], 98)
    part = [None] + [chunks[i].tobytes() for i in range(1, t)]
    expected = [[dig[i].tobytes() for i in range(t)]]
    want = _strip(ce.parts_read(rs, [part], expected))
    # a slot that a batch fills exactly, and one that the same batch exceeds by 16 bytes
    exact = ce.PartsReader(rs, t * _stride(L), 1, 1)
    slot, _ = exact.acquire()
    exact.submit_from(slot, [part], expected)
    assert _strip(exact.collect(slot)) == want and want[0][0][0] == chunks[0].tobytes()
    short = ce.PartsReader(rs, t * _stride(L) - 16, 1, 1)
    slot, stage = short.acquire()
    flags = bytes([0] + [1] * (t - 1))
    for call in (lambda: short.submit_from(slot, [part], expected),
                 lambda: short.submit(slot, [L], flags, b"".join(expected[0]))):
        with pytest.raises(ce.Error) as e:
            call()
        assert e.value.code == ce.ERR_INVALID_ARGUMENT and "slot_bytes" in str(e.value)
    # refused batches leave the slot usable: too many parts, a zero length, then a batch
    (c2, d2), = _oracle_parts(d, p, [4080], 97)
    small = [c2[i].tobytes() for i in range(t - 1)] + [None]
    exp2 = [[d2[i].tobytes() for i in range(t)]]
    for call, code in ((lambda: short.submit_from(slot, [small, small], exp2 * 2),
                        ce.ERR_INVALID_ARGUMENT),
                       (lambda: short.submit(slot, [16, 16], bytes(2 * t), bytes(64 * t)),
                        ce.ERR_INVALID_ARGUMENT),
                       (lambda: short.submit(slot, [0], flags, b"".join(expected[0])),
                        ce.EMPTY_SHARD)):
        with pytest.raises(ce.Error) as e:
            call()
        assert e.value.code == code
    short.submit_from(slot, [small], exp2)
    got = _strip(short.collect(slot))
    assert got == _strip(ce.parts_read(rs, [small], exp2))
    assert got[2] == [ce.OK] and got[0][0][:d] == [c2[i].tobytes() for i in range(d)]
    # null arrays with parts to read, a slot out of range
    lib, one = ce._lib, (ctypes.c_size_t * 1)(16)
    f1, e1 = (ctypes.c_uint8 * t)(), (ctypes.c_uint8 * (32 * t))()
    assert lib.cec_parts_reader_submit(short._h, slot, None, 1, f1, e1) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_submit(short._h, slot, one, 1, None, e1) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_submit(short._h, slot, one, 1, f1, None) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_submit(short._h, 1, one, 1, f1, e1) == ce.ERR_INVALID_ARGUMENT
    assert lib.cec_parts_reader_submit_from(short._h, slot, None, one, 1, f1, e1) == \
        ce.ERR_INVALID_ARGUMENT
    assert _strip(short.collect(slot)) == got  # the slot's batch is untouched by the refusals


def test_empty_batch_query_and_drain(reference):
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    rd = ce.PartsReader(rs, SLOT, MAX_PARTS, DEPTH)
    assert rd.query(0) and rd.query(1)  # nothing in flight
    verified, status, rebuilt, offsets = rd.wait(0)  # a slot with no batch: no parts, at once
    assert verified.shape == (0,) and status.shape == (0,) and rebuilt.shape == (0,)
    assert list(offsets) == [0]
    rd.drain()
    slot, _ = rd.acquire()
    rd.submit_from(slot, [], [])
    rd.submit(slot, [], b"", b"")
    assert rd.query(slot)
    assert list(rd.wait(slot)[3]) == [0] and rd.collect(slot) == ([], b"", [])
    b4, b5 = (_batch(d, p, reference[(d, p)][b], b) for b in (4, 5))
    slot, _ = rd.acquire()
    rd.submit_from(slot, *b4)
    assert rd.query(slot) in (True, False)  # never blocks, whatever the batch's state
    other, _ = rd.acquire()
    rd.submit_from(other, *b5)
    rd.drain()
    assert rd.query(slot) and rd.query(other)
    assert _strip(rd.collect(slot)) == _strip(ce.parts_read(rs, *b4))
    assert _strip(rd.collect(other)) == _strip(ce.parts_read(rs, *b5))
    for call in (lambda: rd.query(DEPTH), lambda: rd.wait(DEPTH),
                 lambda: rd.submit(DEPTH, [16], bytes(5), bytes(160))):
        with pytest.raises(ce.Error) as e:
            call()
        assert e.value.code == ce.ERR_INVALID_ARGUMENT


def test_two_threads_each_with_a_reader_on_one_codec(reference):
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    batches = [_batch(d, p, reference[(d, p)][b], b) for b in range(BATCHES)]
    want = [_strip(ce.parts_read(rs, *bt)) for bt in batches]
    readers = [ce.PartsReader(rs, SLOT, MAX_PARTS, DEPTH) for _ in range(2)]  # made up front
    errors = []

    def run(rd, order):
        try:
            assert _stream(rd, [batches[b] for b in order]) == [want[b] for b in order]
        except BaseException as exc:  # noqa: BLE001  (reported by the main thread)
            errors.append(exc)
    threads = [threading.Thread(target=run, args=(readers[0], list(range(BATCHES)))),
               threading.Thread(target=run, args=(readers[1], list(range(BATCHES))[::-1]))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


@MODES
@pytest.mark.parametrize("d,p", SHAPES)
def test_stats_count_exactly_what_came_back(d, p, data_only, reference):
    t = d + p
    rs = ce.ReedSolomon(d, p)
    rd = ce.PartsReader(rs, SLOT, MAX_PARTS, DEPTH, data_only)
    assert rd.stats() == (0, 0, 0)

    def returned(parts, waited):
        verified, status, _, offsets = waited
        lens = _lens(parts)
        n_out = [sum(1 for i in range(t) if not verified[k * t + i] and (i < d or not data_only))
                 if status[k] == ce.OK else 0 for k in range(len(parts))]
        total = sum(r * _stride(L) for r, L in zip(n_out, lens))
        assert int(offsets[-1]) == total
        return total

    # only known erasures: the host's guess is the whole return, to the byte
    parts, expected = _batch(d, p, reference[(d, p)][6], 6)
    slot, _ = rd.acquire()
    rd.submit_from(slot, parts, expected)
    total = returned(parts, rd.wait(slot))
    loaded = sum(len(c[0] if isinstance(c, tuple) else c) for row in parts for c in row
                 if c is not None)
    assert total > 0
    assert rd.stats() == (len(parts) * t * 32 + loaded, total, 0)
    assert _strip(rd.collect(slot)) == _strip(ce.parts_read(rs, parts, expected, data_only))
    assert rd.stats()[1:] == (total, 0)  # waiting again fetches nothing again
    # one corrupt loaded data chunk in a part with a spare: more comes back than was guessed,
    # through one tail copy, and the bytes are right
    q, i = next((q, i) for q, row in enumerate(parts) if sum(c is None for c in row) < p
                for i in range(d) if isinstance(row[i], bytes))
    parts2, expected2 = _batch(d, p, reference[(d, p)][6], 6, flip={(q, i)})
    assert [[c is None for c in row] for row in parts2] == [[c is None for c in row] for row in parts]
    slot, _ = rd.acquire()
    rd.submit_from(slot, parts2, expected2)
    waited = rd.wait(slot)
    total2 = returned(parts2, waited)
    assert waited[0][q * t + i] == 0 and waited[1][q] == ce.OK
    assert total2 == total + _stride(_lens(parts)[q])
    assert rd.stats()[1:] == (total + total2, 1)
    got = _strip(rd.collect(slot))
    assert got == _strip(ce.parts_read(rs, parts2, expected2, data_only))
    _check_original(d, data_only, reference[(d, p)][6], got)
    assert rd.stats()[1:] == (total + total2, 1)
