"""Segmented ragged writes on the GPU (cec_encode_hash_segments, sha256_resume_kernel): parts go
through as column segments, one per call, their SHA-256 chains resumed from midstate records in
device memory.  Every comparison is exact and against the WHOLE part: the CPU oracle's parity of
the whole part, cut at the segment's columns, and hashlib.sha256 of the whole chunk.  Both regions
of every call, its digest rows and the midstate pool lie in canary bytes that are checked after
every call: exactly seg_len bytes of each parity piece are written, digest rows only for entries
that end their part, and nothing around the pool."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import CANARY, DEV, _oracle_parts, _stride  # noqa: E402

SHAPES = [(3, 2), (10, 4)]
# one or two tail blocks, a padding-only tail (a multiple of 64), a one-byte last segment
LENGTHS = [1, 55, 56, 63, 64, 65, 119, 120, 128, 129, 191, 192, 193, 320]
SEGMENTS = [64, 128, 192]  # odd and even full-block counts: both arms of the paired load
GUARD = 64
F, L_ = ce.SEG_FIRST, ce.SEG_LAST


@pytest.fixture(scope="module")
def reference():
    """Per shape: ten parts of every chunk length (140 parts), from the CPU oracle, with hashlib's
    digest of every whole chunk.  Computed once, shared, never modified."""
    out = {}
    for d, p in SHAPES:
        parts = _oracle_parts(d, p, LENGTHS * 10, 100 * d + p)
        dig = [[hashlib.sha256(c.tobytes()).digest() for c in list(data) + list(par)]
               for data, par, _ in parts]
        out[(d, p)] = (parts, dig)
    return out


class Pool:
    """A midstate pool of n_slots * t records between two guards of canary bytes."""

    def __init__(self, n_slots, t):
        assert ce.MIDSTATE_BYTES == 48
        self.n_slots = n_slots
        self.bytes = n_slots * t * 48
        self.buf = torch.full((self.bytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def guards_intact(self):
        host = self.buf.cpu().numpy()
        return bool((host[:GUARD] == CANARY).all() and (host[GUARD + self.bytes:] == CANARY).all())


def _call(rs, ref, entries, pool):
    """One cec_encode_hash_segments call.  entries: (part, column offset, seg_len, slot).  Checks
    the whole of both regions, every digest row and the pool's guards; returns the parity region
    and the digests as numpy arrays (for the byte-for-byte comparisons)."""
    parts, dig = ref
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    t = d + p
    segs = [e[2] for e in entries]
    doffs, poffs, db, pb = ce.split_layout(d, p, segs)
    data_in = np.full(db + GUARD, CANARY, np.uint8)
    want_par = np.full(pb + GUARD, CANARY, np.uint8)
    want_dig = np.full((len(entries), t, 32), CANARY, np.uint8)
    flags = []
    for k, ((q, off, seg, _), do, po) in enumerate(zip(entries, doffs, poffs)):
        data, par, _ = parts[q]
        L = data.shape[1]
        assert 0 < seg and off + seg <= L
        fl = (F if off == 0 else 0) | (L_ if off + seg == L else 0)
        flags.append(fl)
        for j in range(d):
            data_in[do + j * _stride(seg):do + j * _stride(seg) + seg] = data[j][off:off + seg]
        for i in range(p):
            want_par[po + i * _stride(seg):po + i * _stride(seg) + seg] = par[i][off:off + seg]
        if fl & L_:
            for i in range(t):
                want_dig[k, i] = np.frombuffer(dig[q][i], np.uint8)
    dbuf = torch.from_numpy(data_in).to(DEV)
    pbuf = torch.full((pb + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    dg = torch.full((len(entries), t, 32), CANARY, dtype=torch.uint8, device=DEV)
    ce.encode_hash_segments(rs, dbuf.data_ptr(), doffs, pbuf.data_ptr(), poffs, segs,
                            [e[3] for e in entries], flags, pool.ptr if pool else 0,
                            pool.n_slots if pool else 0, dg.data_ptr())
    torch.cuda.synchronize()
    got_par, got_dig = pbuf.cpu().numpy(), dg.cpu().numpy()
    assert np.array_equal(got_par, want_par), "parity pieces, or bytes around them"
    assert np.array_equal(dbuf.cpu().numpy(), data_in), "the data region was written"
    bad = [(entries[k], i) for k in range(len(entries)) for i in range(t)
           if not np.array_equal(got_dig[k, i], want_dig[k, i])]
    assert not bad, f"digest rows (LAST) or canaries (others) differ: {bad[:4]}"
    assert pool is None or pool.guards_intact()
    return got_par, got_dig, flags


def _segments(L, S):
    return [(off, min(S, L - off)) for off in range(0, L, S)]


@pytest.mark.parametrize("S", SEGMENTS)
@pytest.mark.parametrize("d,p", SHAPES)
def test_each_chunk_through_successive_calls(d, p, S, reference):
    """Every chunk length through ceil(L / S) calls on one stream: call r holds segment r of every
    part that has one."""
    rs = ce.ReedSolomon(d, p)
    ref = reference[(d, p)]
    n = len(LENGTHS)
    pool = Pool(n, d + p)
    ended = 0
    for r in range(-(-max(LENGTHS) // S)):
        entries = [(q, *_segments(L, S)[r], q) for q, L in enumerate(LENGTHS)
                   if r < len(_segments(L, S))]
        _, _, flags = _call(rs, ref, entries, pool)
        ended += sum(1 for f in flags if f & L_)
    assert ended == n


@pytest.mark.parametrize("d,p", SHAPES)
def test_one_batch_mixes_first_middle_last_and_whole(d, p, reference):
    """140 parts started over three calls, so that one call holds FIRST, middle, LAST and
    FIRST|LAST entries of different parts: more than 60 entries (over 256 items, two workgroups),
    in shuffled entry order and with shuffled slots."""
    rs = ce.ReedSolomon(d, p)
    ref = reference[(d, p)]
    S = 64
    n = len(ref[0])
    rng = np.random.default_rng(7 * d + p)
    slot = rng.permutation(n)
    pool = Pool(n, d + p)
    plan = {}
    for q in range(n):
        for r, (off, seg) in enumerate(_segments(LENGTHS[q % len(LENGTHS)], S)):
            plan.setdefault(q % 3 + r, []).append((q, off, seg, int(slot[q])))
    mixed = ended = 0
    for r in sorted(plan):
        entries = [plan[r][k] for k in rng.permutation(len(plan[r]))]
        _, _, flags = _call(rs, ref, entries, pool)
        ended += sum(1 for f in flags if f & L_)
        if set(flags) == {0, F, L_, F | L_} and len(entries) >= 60:
            assert len(entries) * (d + p) > 256
            mixed += 1
    assert mixed >= 1 and ended == n


@pytest.mark.parametrize("d,p", SHAPES)
def test_whole_parts_equal_encode_hash_split(d, p, reference):
    """A batch of FIRST|LAST entries touches no record (no pool at all) and gives, byte for byte,
    what cec_encode_hash_split gives."""
    rs = ce.ReedSolomon(d, p)
    ref = reference[(d, p)]
    n = len(LENGTHS)
    entries = [(q, 0, L, 0xFFFFFFFF) for q, L in enumerate(LENGTHS)]  # the slot is ignored
    got_par, got_dig, flags = _call(rs, ref, entries, None)
    assert set(flags) == {F | L_}
    doffs, poffs, db, pb = ce.split_layout(d, p, LENGTHS)
    data_in = np.full(db + GUARD, CANARY, np.uint8)
    for q, (do, L) in enumerate(zip(doffs, LENGTHS)):
        for j in range(d):
            data_in[do + j * _stride(L):do + j * _stride(L) + L] = ref[0][q][0][j]
    dbuf = torch.from_numpy(data_in).to(DEV)
    pbuf = torch.full((pb + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    dg = torch.full((n, d + p, 32), CANARY, dtype=torch.uint8, device=DEV)
    ce.encode_hash_split(rs, dbuf.data_ptr(), doffs, pbuf.data_ptr(), poffs, LENGTHS,
                         dg.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(pbuf.cpu().numpy(), got_par)
    assert np.array_equal(dg.cpu().numpy(), got_dig)


def test_a_slot_serves_another_part_right_after_its_last(reference):
    """One state slot: part A's LAST in one call, part B's FIRST on the same slot in the next."""
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    ref = reference[(d, p)]
    pool = Pool(1, d + p)
    a, b = LENGTHS.index(193), LENGTHS.index(320)
    for q in (a, b, a):
        for off, seg in _segments(LENGTHS[q], 64):
            _call(rs, ref, [(q, off, seg, 0)], pool)


def test_calls_queued_back_to_back_on_one_stream(reference):
    """The segments of a part queued without a wait between the calls: the stream orders them."""
    d, p = 10, 4
    t = d + p
    rs = ce.ReedSolomon(d, p)
    parts, dig = reference[(d, p)]
    q = LENGTHS.index(320)
    data = parts[q][0]
    pool = Pool(1, t)
    keep, rows = [], None
    for off, seg in _segments(320, 128):
        doffs, poffs, db, pb = ce.split_layout(d, p, [seg])
        host = np.zeros(db, np.uint8)
        for j in range(d):
            host[j * _stride(seg):j * _stride(seg) + seg] = data[j][off:off + seg]
        dbuf = torch.from_numpy(host).to(DEV)
        pbuf = torch.zeros(pb, dtype=torch.uint8, device=DEV)
        rows = torch.full((1, t, 32), CANARY, dtype=torch.uint8, device=DEV)
        keep.append((dbuf, pbuf, rows))
        fl = (F if off == 0 else 0) | (L_ if off + seg == 320 else 0)
        ce.encode_hash_segments(rs, dbuf.data_ptr(), doffs, pbuf.data_ptr(), poffs, [seg], [0],
                                [fl], pool.ptr, 1, rows.data_ptr())
    torch.cuda.synchronize()
    assert [bytes(r) for r in rows.cpu().numpy()[0]] == dig[q]
    assert pool.guards_intact()
