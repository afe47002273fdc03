"""The segment pipeline on the GPU (cec_segment_pipeline_*): parts of different sizes stream through
small slots as column segments, long parts over three and more batches while short ones come and
go, the midstates of the open parts kept on the device and their ids reused.  The assembled parity
of every part is compared with the CPU oracle's parity of the WHOLE part and every digest with
hashlib.sha256 of the WHOLE chunk; all exact."""
import ctypes
import hashlib

import numpy as np
import pytest

from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
import oracle  # noqa: E402

SEG = 128
SLOT = 8192  # bytes of padded data per batch
# chunk lengths: whole parts, parts of two segments, and parts of three to six (one an exact
# multiple of the segment, one with a one-byte last segment)
CHUNKS = [700, 1, 64, 300, 129, 384, 17, 128, 513, 256, 90, 385, 127, 640, 2, 257]


def _stride(L):
    return (L + 15) // 16 * 16


@pytest.fixture(scope="module")
def reference():
    """Per shape: 32 parts (lengths a few bytes short of d * L, so the last data chunk is padded),
    the oracle's parity and hashlib's digests of all d + p chunks.  Computed once, never modified."""
    out = {}
    for d, p in ((3, 2), (10, 4)):
        parts = []
        for q, L in enumerate(CHUNKS * 2):
            length = d * L - (q % min(L, 3))
            buf = gen_bytes(31 * d + q, length)
            cs, par, _ = oracle.part_encode(d, p, buf, length)
            assert cs == L
            padded = np.zeros(d * L, np.uint8)
            padded[:length] = buf
            dig = [hashlib.sha256(padded[j * L:(j + 1) * L].tobytes()).digest() for j in range(d)]
            dig += [hashlib.sha256(par[i].tobytes()).digest() for i in range(p)]
            parts.append((buf, L, par, dig))
        out[(d, p)] = parts
    return out


class Driver:
    """Feeds parts through a SegmentPipeline: each batch takes the next segment of every open
    part, then new parts while the slot, max_parts and the ids last.  Up to `depth` batches are in
    flight; a slot's results are collected just before the slot is acquired again."""

    def __init__(self, rs, depth, max_open, max_parts=12):
        self.d, self.p = rs.data_shard_count(), rs.parity_shard_count()
        self.pl = ce.SegmentPipeline(rs, SLOT, max_parts, depth, max_open)
        self.max_parts = max_parts
        self.free_ids = list(range(max_open))[::-1]
        self.ids_given = []
        self.open = []      # [part index, columns done, id]
        self.in_flight = []  # (slot, entries: (part index, off, seg, last))
        self.parity, self.digests, self.batches = {}, {}, {}

    def _collect(self):
        slot, entries = self.in_flight.pop(0)
        parity, digests = self.pl.wait(slot)
        assert digests.shape[0] == len(entries)
        _, poffs, _, pb = ce.split_layout(self.d, self.p, [e[2] for e in entries])
        assert parity.size == pb
        for k, ((q, off, seg, last), po) in enumerate(zip(entries, poffs)):
            for i in range(self.p):
                self.parity[q][i, off:off + seg] = parity[po + i * _stride(seg):][:seg]
            if last:
                self.digests[q] = [bytes(r) for r in digests[k]]

    def run(self, parts):
        todo = list(range(len(parts)))
        while todo or self.open:
            batch, room = [], SLOT
            for o in self.open:
                q, done, oid = o
                seg = min(SEG, parts[q][1] - done)
                if len(batch) < self.max_parts and room >= self.d * _stride(seg):
                    batch.append((q, done, seg, oid))
                    room -= self.d * _stride(seg)
            while todo and len(batch) < self.max_parts:
                q = todo[0]
                L = parts[q][1]
                seg = min(SEG, L)
                if room < self.d * _stride(seg) or (L > SEG and not self.free_ids):
                    break
                oid = 0xFFFFFFFF  # a whole part's id is ignored
                if L > SEG:
                    oid = self.free_ids.pop()
                    self.ids_given.append(oid)
                    self.open.append([q, 0, oid])
                self.parity[q] = np.zeros((self.p, L), np.uint8)
                batch.append((q, 0, seg, oid))
                room -= self.d * _stride(seg)
                todo.pop(0)
            assert batch
            if len(self.in_flight) == self.pl.depth:
                self._collect()
            slot = self.pl.acquire()
            cs = self.pl.submit_from(slot, [(parts[q][0], off, seg, oid)
                                            for q, off, seg, oid in batch])
            assert cs == [parts[q][1] for q, _, _, _ in batch]
            self.in_flight.append((slot, [(q, off, seg, off + seg == parts[q][1])
                                          for q, off, seg, _ in batch]))
            for q, off, seg, _ in batch:
                self.batches[q] = self.batches.get(q, 0) + 1
            for o in list(self.open):
                hit = [b for b in batch if b[0] == o[0]]
                if hit:
                    o[1] = hit[0][1] + hit[0][2]
                    if o[1] == parts[o[0]][1]:
                        self.open.remove(o)
                        self.free_ids.append(o[2])
        while self.in_flight:
            self._collect()


@pytest.mark.parametrize("depth,max_open", [(2, 3), (3, 2)])
@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_long_parts_span_batches_while_short_ones_come_and_go(d, p, depth, max_open, reference):
    rs = ce.ReedSolomon(d, p)
    parts = reference[(d, p)]
    drv = Driver(rs, depth, max_open)
    assert drv.pl.depth == depth == ce._lib.cec_segment_pipeline_depth(drv.pl._h)
    drv.run(parts)
    assert drv.pl.open_count() == 0
    drv.pl.drain()
    for q, (_, L, par, dig) in enumerate(parts):
        assert np.array_equal(drv.parity[q], par), (q, L, "parity")
        assert drv.digests[q] == dig, (q, L, "digests")
        assert drv.batches[q] == -(-L // SEG)
    assert max(drv.batches.values()) >= 3
    assert len(drv.ids_given) > max_open  # ids were reused
    assert all(drv.pl.query(s) for s in range(depth))


def test_only_whole_parts_without_a_pool(reference):
    """max_open == 0: every part is one entry, no id is ever looked at."""
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    parts = [x for x in reference[(d, p)] if x[1] <= SEG]
    drv = Driver(rs, 2, 0)
    drv.run(parts)
    for q, (_, L, par, dig) in enumerate(parts):
        assert np.array_equal(drv.parity[q], par) and drv.digests[q] == dig, (q, L)
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
    ]
    cs = (ctypes.c_size_t * m)()
    args = [None if i in null else a for i, a in enumerate(args)]
    return ce._lib.cec_segment_pipeline_submit_from(pl._h, slot, *args, n, None if 5 in null else cs)


def test_abandon_frees_an_id_and_refusals_leave_everything_as_it_was(reference):
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    parts = reference[(d, p)]
    long_q = CHUNKS.index(700)
    buf, L, par, dig = parts[long_q]
    other, L2, _, dig2 = parts[CHUNKS.index(513)]
    buf, other = buf.tobytes(), other.tobytes()
    big = other * 12
    pl = ce.SegmentPipeline(rs, SLOT, 4, 2, 2)
    INV = ce.ERR_INVALID_ARGUMENT
    slot = pl.acquire()
    pl.submit_from(slot, [(buf, 0, SEG, 1)])
    assert pl.open_count() == 1
    slot = pl.acquire()
    # the parts pipeline's own refusals first
    for null in range(6):
        assert _raw(pl, slot, [(buf, SEG, SEG, 1)], null=(null,)) == INV, null
    assert _raw(pl, 2, [(buf, SEG, SEG, 1)]) == INV
    assert _raw(pl, slot, [(buf, SEG, SEG, 1)] * 5) == INV  # n > max_parts
    assert _raw(pl, slot, [(buf, SEG, 0, 1)]) == ce.EMPTY_SHARD
    assert _raw(pl, slot, [(b"", SEG, SEG, 1)]) == ce.EMPTY_SHARD
    # then the segment rules, in the header's order: an entry that breaks a rule and every later one
    refused = [
        [(other, 0, 100, 2)],                          # id >= max_open (and not a multiple of 64)
        [(buf, SEG, SEG, 1), (other, 0, 100, 1)],      # an id twice (and the second one's length)
        [(other, 0, 100, 1)],                          # FIRST on an open id
        [(other, SEG, 100, 0)],                        # a continuation on an id that is not open
        [(buf, 2 * SEG, 1000, 1)],                     # not the columns so far (and past L)
        [(buf, SEG, 1000, 1)],                         # past L
        [(buf, SEG, 100, 1)],                          # not LAST and no multiple of 64
        [(buf, SEG, SEG, 1), (other, 0, L2, 0)] * 2,   # the same entries twice
        [(big, 0, -(-len(big) // d), 7)],              # a whole part beyond the slot's capacity
    ]
    for entries in refused:
        assert _raw(pl, slot, entries) == INV, entries
        assert ce._lib.cec_last_error()
        assert pl.open_count() == 1
    # the slot is usable and the chain is where it was: the part goes on and ends right
    got = np.zeros((p, L), np.uint8)
    pl.submit_from(slot, [(buf, SEG, SEG, 1)])
    off = 2 * SEG
    while off < L:
        seg = min(SEG, L - off)
        s = pl.acquire()
        pl.submit_from(s, [(buf, off, seg, 1)])
        parity, digests = pl.wait(s)
        got[:, off:off + seg] = np.stack([parity[i * _stride(seg):][:seg] for i in range(p)])
        off += seg
    assert pl.open_count() == 0
    assert [bytes(r) for r in digests[0]] == dig
    assert np.array_equal(got[:, 2 * SEG:], par[:, 2 * SEG:])
    # abandon: an open id is closed, its chain gone, and it serves another part
    s = pl.acquire()
    pl.submit_from(s, [(buf, 0, SEG, 0)])
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
        pl.submit_from(s, [(other, off, seg, 0)])
        off += seg
    _, digests = pl.wait(s)
    assert [bytes(r) for r in digests[0]] == dig2
    assert pl.open_count() == 0
