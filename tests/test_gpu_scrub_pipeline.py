"""The scrub pipeline on the GPU (cec_scrub_pipeline_*): stored copies of different sizes stream
through small slots as segments, long copies over many batches while short ones come and go, the
midstates of the open copies kept on the device and their ids reused.  Every flag is compared with
hashlib.sha256 of the WHOLE copy against its expected digest, and with cec_parts_verify's flag for
the same list."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)

LENGTHS = [1, 55, 56, 63, 64, 65, 119, 120, 128, 129, 191, 192, 193, 320]
SLOT = 2048  # bytes of padded segments per batch: dozens of batches for the copies below
MAX_ENTRIES = 12
INV = ce.ERR_INVALID_ARGUMENT


def _stride(L):
    return (L + 15) // 16 * 16


@pytest.fixture(scope="module")
def reference():
    """196 copies over the LENGTHS cycle and a few of 4097 and 16385 bytes; roughly one in five is
    damaged (one bit of one byte, first, middle or last), so its stored bytes no longer hash to its
    expected digest.  With hashlib's verdicts and cec_parts_verify's flags for the same list.
    Computed once, shared, never modified."""
    rng = np.random.default_rng(2024)
    lens = [LENGTHS[q % len(LENGTHS)] for q in range(196)]
    for at, L in ((17, 4097), (60, 16385), (61, 4097), (150, 16385), (195, 4097)):
        lens.insert(at, L)
    copies, expected = [], []
    for q, L in enumerate(lens):
        good = rng.integers(0, 256, L, dtype=np.uint8)
        expected.append(hashlib.sha256(good.tobytes()).digest())
        if q % 5 == 3:
            good = good.copy()
            good[(0, L // 2, L - 1)[q % 3]] ^= 1 << (q % 8)
        copies.append(good.tobytes())
    verdict = [int(hashlib.sha256(c).digest() == e) for c, e in zip(copies, expected)]
    assert 30 < verdict.count(0) < 50 and verdict[60] == 1 and verdict[153] == 0
    one_call = list(ce.parts_verify(copies, expected))
    return copies, expected, verdict, one_call


class Driver:
    """Feeds copies through a ScrubPipeline: each batch takes the next segment of every open copy,
    then new copies while the slot, max_entries and the ids last.  Up to `depth` batches are in
    flight; a slot's results are collected just before the slot is acquired again."""

    def __init__(self, seg, depth, max_open):
        self.seg = seg
        self.pl = ce.ScrubPipeline(SLOT, MAX_ENTRIES, depth, max_open)
        self.free_ids = list(range(max_open))[::-1]
        self.ids_given = []
        self.open = []       # [copy index, bytes done, id]
        self.in_flight = []  # (slot, entries: (copy index, last))
        self.ok, self.batches, self.n_batches, self.most_open = {}, {}, 0, 0

    def _collect(self):
        slot, entries = self.in_flight.pop(0)
        ok = self.pl.wait(slot)
        assert ok.shape == (len(entries),)
        for k, (q, last) in enumerate(entries):
            if last:
                assert q not in self.ok
                self.ok[q] = int(ok[k])

    def run(self, copies, expected):
        todo = list(range(len(copies)))
        while todo or self.open:
            batch, room = [], SLOT
            for q, done, oid in self.open:
                seg = min(self.seg, len(copies[q]) - done)
                if len(batch) < MAX_ENTRIES and room >= _stride(seg):
                    batch.append((q, done, seg, oid))
                    room -= _stride(seg)
            while todo and len(batch) < MAX_ENTRIES:
                q = todo[0]
                L = len(copies[q])
                seg = min(self.seg, L)
                if room < _stride(seg) or (L > self.seg and not self.free_ids):
                    break
                oid = 0xFFFFFFFF  # a whole copy's id is ignored
                if L > self.seg:
                    oid = self.free_ids.pop()
                    self.ids_given.append(oid)
                    self.open.append([q, 0, oid])
                batch.append((q, 0, seg, oid))
                room -= _stride(seg)
                todo.pop(0)
            assert batch
            if len(self.in_flight) == self.pl.depth:
                self._collect()
            slot = self.pl.acquire()
            # the digest goes along only where the copy ends: the other rows are never read
            self.pl.submit_from(slot, [
                (copies[q], off, seg, oid, expected[q] if off + seg == len(copies[q]) else None)
                for q, off, seg, oid in batch])
            self.n_batches += 1
            self.in_flight.append((slot, [(q, off + seg == len(copies[q]))
                                          for q, off, seg, _ in batch]))
            for q, off, seg, _ in batch:
                self.batches[q] = self.batches.get(q, 0) + 1
            for o in list(self.open):
                hit = [b for b in batch if b[0] == o[0]]
                if hit:
                    o[1] = hit[0][1] + hit[0][2]
                    if o[1] == len(copies[o[0]]):
                        self.open.remove(o)
                        self.free_ids.append(o[2])
            assert self.pl.open_count() == len(self.open)
            self.most_open = max(self.most_open, len(self.open))
        while self.in_flight:
            self._collect()


@pytest.mark.parametrize("depth,max_open", [(1, 3), (2, 1), (3, 64), (3, 3)])
@pytest.mark.parametrize("seg", [64, 192])
def test_flags_equal_hashlib_and_parts_verify(seg, depth, max_open, reference):
    copies, expected, verdict, one_call = reference
    drv = Driver(seg, depth, max_open)
    assert drv.pl.depth == depth == ce._lib.cec_scrub_pipeline_depth(drv.pl._h)
    drv.run(copies, expected)
    assert drv.pl.open_count() == 0
    drv.pl.drain()
    got = [drv.ok[q] for q in range(len(copies))]
    assert got == verdict
    assert got == one_call
    for q, c in enumerate(copies):
        assert drv.batches[q] == -(-len(c) // seg), q
    assert drv.n_batches >= 24 and max(drv.batches.values()) >= 86  # 16385 bytes in 192s
    assert 1 <= drv.most_open <= max_open
    assert len(drv.ids_given) > max_open or max_open == 64  # ids were reused
    assert all(drv.pl.query(s) for s in range(depth))


def test_only_whole_copies_without_a_pool(reference):
    """max_open == 0: every copy is one entry, no id is ever looked at."""
    copies, expected, verdict, _ = reference
    short = [q for q, c in enumerate(copies) if len(c) <= 192]
    drv = Driver(192, 2, 0)
    drv.run([copies[q] for q in short], [expected[q] for q in short])
    assert [drv.ok[x] for x in range(len(short))] == [verdict[q] for q in short]
    assert drv.pl.open_count() == 0


def _raw(pl, slot, entries, null=()):
    n = len(entries)
    keep = []
    m = max(n, 1)
    args = [
        (ce._u8p * m)(*[ce._buf_ptr(e[0], keep) for e in entries]),
        (ctypes.c_size_t * m)(*[len(e[0]) for e in entries]),
        (ctypes.c_size_t * m)(*[e[1] for e in entries]),
        (ctypes.c_size_t * m)(*[e[2] for e in entries]),
        (ctypes.c_uint32 * m)(*[e[3] for e in entries]),
        (ctypes.c_uint8 * (32 * m))(),
    ]
    args = [None if i in null else a for i, a in enumerate(args)]
    return ce._lib.cec_scrub_pipeline_submit_from(pl._h, slot, *args, n)


def test_abandon_frees_an_id_and_refusals_leave_everything_as_it_was(reference):
    copies, expected, verdict, _ = reference
    SEG = 128
    long_q, other_q = 17, 61  # 4097 bytes each, both good
    assert verdict[long_q] == verdict[other_q] == 1
    buf, other = copies[long_q], copies[other_q]
    L, L2 = len(buf), len(other)
    pl = ce.ScrubPipeline(SLOT, 4, 2, 2)
    slot = pl.acquire()
    pl.submit_from(slot, [(buf, 0, SEG, 1, None)])
    assert pl.open_count() == 1
    slot = pl.acquire()
    # the call's own refusals first
    for null in range(6):
        assert _raw(pl, slot, [(buf, SEG, SEG, 1)], null=(null,)) == INV, null
    assert _raw(pl, 2, [(buf, SEG, SEG, 1)]) == INV
    assert _raw(pl, slot, [(buf, SEG, SEG, 1)] * 5) == INV  # n > max_entries
    assert _raw(pl, slot, [(buf, SEG, 0, 1)]) == ce.EMPTY_SHARD
    assert _raw(pl, slot, [(b"", SEG, SEG, 1)]) == ce.EMPTY_SHARD
    # then the segment rules, in the header's order: an entry that breaks a rule and every later one
    refused = [
        [(other, 0, 100, 2)],                          # id >= max_open (and not a multiple of 64)
        [(buf, SEG, SEG, 1), (other, 0, 100, 1)],      # an id twice (and the second one's length)
        [(other, 0, 100, 1)],                          # FIRST on an open id
        [(other, SEG, 100, 0)],                        # a continuation on an id that is not open
        [(buf, 2 * SEG, 5000, 1)],                     # not the bytes so far (and past L)
        [(buf, SEG, 5000, 1)],                         # past L
        [(buf, SEG, 100, 1)],                          # not LAST and no multiple of 64
        [(buf, SEG, SEG, 1), (copies[0], 0, 1, 0)] * 2,  # the same entries twice
        [(other, 0, L2, 7)],                           # a whole copy beyond the slot's capacity
        [(buf, SEG, 2112, 1)],                         # a segment beyond the slot's capacity
    ]
    for entries in refused:
        assert _raw(pl, slot, entries) == INV, entries
        assert ce._lib.cec_last_error()
        assert pl.open_count() == 1
    assert b"slot_bytes" in ce._lib.cec_last_error()
    # the slot is usable and the chain is where it was: the copy goes on and ends right, beside a
    # damaged whole copy in its last batch
    pl.submit_from(slot, [(buf, SEG, SEG, 1, None)])
    off = 2 * SEG
    while off < L:
        seg = min(SEG, L - off)
        s = pl.acquire()
        pl.submit_from(s, [(buf, off, seg, 1, expected[long_q]), (copies[3], 0, len(copies[3]), 9,
                                                                 expected[3])])
        off += seg
    ok = pl.wait(s)
    assert pl.open_count() == 0
    assert list(ok) == [1, 0] and verdict[3] == 0
    # abandon: an open id is closed, its chain gone, and it serves another copy
    s = pl.acquire()
    pl.submit_from(s, [(buf, 0, SEG, 0, None)])
    assert pl.open_count() == 1
    with pytest.raises(ce.Error):
        pl.abandon(1)
    pl.abandon(0)
    assert pl.open_count() == 0
    with pytest.raises(ce.Error):
        pl.abandon(0)
    assert _raw(pl, pl.acquire(), [(buf, SEG, SEG, 0)]) == INV
    off = 0
    while off < L2:
        seg = min(SEG, L2 - off)
        s = pl.acquire()
        pl.submit_from(s, [(other, off, seg, 0, expected[other_q])])
        off += seg
    assert list(pl.wait(s)) == [1]
    assert pl.open_count() == 0
    # an empty batch is a batch of nothing
    s = pl.acquire()
    pl.submit_from(s, [])
    assert pl.wait(s).shape == (0,)
