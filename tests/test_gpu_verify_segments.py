"""The segmented scrub on the GPU (cec_verify_segments, sha256_resume_verify_kernel): stored copies
go through as segments, one per call, their SHA-256 chains resumed from midstate records in device
memory, and where a copy ends one flag says whether the WHOLE copy has the expected digest.  The
truth is hashlib.sha256 of the whole copy.  Every call has the ok bytes, the midstate pool and the
segments' region between canary bytes, all checked whole after the call: ok bytes are written for
entries that end their copy only, nothing around the pool, and the region is never written."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import CANARY, DEV  # noqa: E402

# one or two tail blocks, a padding-only tail (a multiple of 64), a one-byte last segment
LENGTHS = [1, 55, 56, 63, 64, 65, 119, 120, 128, 129, 191, 192, 193, 320]
SEGMENTS = [64, 128, 192]  # odd and even full-block counts: both arms of the paired load
GUARD = 64
F, L_ = ce.SEG_FIRST, ce.SEG_LAST


@pytest.fixture(scope="module")
def reference():
    """300 copies over the LENGTHS cycle with hashlib's digest of each whole copy.  Computed once,
    shared, never modified."""
    rng = np.random.default_rng(48)
    copies = [rng.integers(0, 256, LENGTHS[q % len(LENGTHS)], dtype=np.uint8) for q in range(300)]
    digests = [hashlib.sha256(c.tobytes()).digest() for c in copies]
    return copies, digests


class Pool:
    """A midstate pool of n_slots records between two guards of canary bytes."""

    def __init__(self, n_slots):
        assert ce.MIDSTATE_BYTES == 48
        self.n_slots = n_slots
        self.bytes = n_slots * 48
        self.buf = torch.full((self.bytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def guards_intact(self):
        host = self.buf.cpu().numpy()
        return bool((host[:GUARD] == CANARY).all() and (host[GUARD + self.bytes:] == CANARY).all())


def _segments(L, S):
    return [(off, min(S, L - off)) for off in range(0, L, S)]


def _stage(ref, entries, damage=None):
    """The device buffers of one call.  entries: (copy, offset, seg_len, slot).  damage: {entry
    index: byte index within its segment} to flip.  Returns (region, offsets, segs, flags, expected
    rows, ok bytes, the region's host image)."""
    copies, digests = ref
    segs = [e[2] for e in entries]
    offs, total = ce.ragged_layout(1, segs)
    image = np.full(GUARD + total + GUARD, CANARY, np.uint8)
    rows = np.full((len(entries), 32), CANARY, np.uint8)
    flags = []
    for k, ((q, off, seg, _), o) in enumerate(zip(entries, offs)):
        L = len(copies[q])
        assert 0 < seg and off + seg <= L
        fl = (F if off == 0 else 0) | (L_ if off + seg == L else 0)
        flags.append(fl)
        image[GUARD + o:GUARD + o + seg] = copies[q][off:off + seg]
        if damage and k in damage:
            image[GUARD + o + damage[k]] ^= 0x10
        if fl & L_:  # rows of other entries stay canary: they are never read
            rows[k] = np.frombuffer(digests[q], np.uint8)
    region = torch.from_numpy(image).to(DEV)
    assert (region.data_ptr() + GUARD) % 16 == 0
    return region, offs, segs, flags, rows, image


def _call(ref, entries, pool, damage=None, rows_edit=None):
    """One cec_verify_segments call, checked whole: returns (flags, ok as numpy).  ok[k] is
    asserted canary for every entry that does not end its copy."""
    region, offs, segs, flags, rows, image = _stage(ref, entries, damage)
    if rows_edit:
        rows_edit(rows)
    exp = torch.from_numpy(rows).to(DEV)
    okb = torch.full((GUARD + len(entries) + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    ce.verify_segments(region.data_ptr() + GUARD, offs, segs, [e[3] for e in entries], flags,
                       pool.ptr if pool else 0, pool.n_slots if pool else 0, exp.data_ptr(),
                       okb.data_ptr() + GUARD)
    torch.cuda.synchronize()
    got = okb.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[GUARD + len(entries):] == CANARY).all()
    ok = got[GUARD:GUARD + len(entries)]
    for k, fl in enumerate(flags):
        if not fl & L_:
            assert ok[k] == CANARY, f"ok byte of entry {k} (not LAST) was touched"
        else:
            assert ok[k] in (0, 1), f"ok byte of LAST entry {k} is {ok[k]}"
    assert np.array_equal(region.cpu().numpy(), image), "the segments' region was written"
    assert np.array_equal(exp.cpu().numpy(), rows), "the expected rows were written"
    assert pool is None or pool.guards_intact()
    return flags, ok


def _last_ok(flags, ok):
    return [int(ok[k]) for k, fl in enumerate(flags) if fl & L_]


@pytest.mark.parametrize("S", SEGMENTS)
def test_each_length_through_successive_calls(S, reference):
    """Every copy length through ceil(L / S) calls on one stream: call r holds segment r of every
    copy that has one; each copy's LAST says 1."""
    n = len(LENGTHS)
    pool = Pool(n)
    ended = 0
    for r in range(-(-max(LENGTHS) // S)):
        entries = [(q, *_segments(L, S)[r], q) for q, L in enumerate(LENGTHS)
                   if r < len(_segments(L, S))]
        flags, ok = _call(reference, entries, pool)
        verdicts = _last_ok(flags, ok)
        assert all(v == 1 for v in verdicts), (S, r, verdicts)
        ended += len(verdicts)
    assert ended == n


def _through(ref, copies_q, S, pool, damage_at=None, rows_edit_at=None):
    """The copies copies_q (slot = position) through successive calls of segments S.  damage_at:
    (position, absolute byte) to flip; rows_edit_at: (position, fn(row)).  Returns {position:
    verdict}."""
    copies, _ = ref
    verdict = {}
    rounds = max(len(_segments(len(copies[q]), S)) for q in copies_q)
    for r in range(rounds):
        entries, pos = [], []
        for x, q in enumerate(copies_q):
            segs = _segments(len(copies[q]), S)
            if r < len(segs):
                entries.append((q, *segs[r], x))
                pos.append(x)
        damage = None
        if damage_at is not None and damage_at[0] in pos:
            k = pos.index(damage_at[0])
            off, seg = entries[k][1], entries[k][2]
            if off <= damage_at[1] < off + seg:
                damage = {k: damage_at[1] - off}
        edit = None
        if rows_edit_at is not None and rows_edit_at[0] in pos:
            k = pos.index(rows_edit_at[0])
            edit = lambda rows, k=k: rows_edit_at[1](rows[k])  # noqa: E731
        flags, ok = _call(ref, entries, pool, damage, edit)
        for k, fl in enumerate(flags):
            if fl & L_:
                verdict[pos[k]] = int(ok[k])
    return verdict


@pytest.mark.parametrize("S", [64, 128])
def test_a_flipped_data_byte_is_caught_and_the_neighbours_stand(S, reference):
    """One byte flipped in a copy's first, middle and last segment and in the tail past the last
    full block: ok == 0 for that copy, 1 for the copies on either side in the same calls."""
    a, b, c = LENGTHS.index(193), LENGTHS.index(320), LENGTHS.index(191)
    pool = Pool(3)
    # 320 bytes: first segment, a middle one, the last, and the last block's bytes; 63 of its
    # neighbours' lengths make the tail cases: 193 = 3 blocks + 1 byte, 191 = 2 blocks + 63
    for victim, byte in ((1, 0), (1, 63), (1, 130), (1, 200), (1, 319), (0, 192), (0, 5),
                         (2, 128), (2, 190), (2, 100)):
        verdict = _through(reference, [a, b, c], S, pool, damage_at=(victim, byte))
        want = {0: 1, 1: 1, 2: 1}
        want[victim] = 0
        assert verdict == want, (S, victim, byte, verdict)
    assert _through(reference, [a, b, c], S, pool) == {0: 1, 1: 1, 2: 1}


def test_every_expected_byte_takes_part_in_the_compare(reference):
    """A 64-byte copy (one full block and a padding-only tail), whole: one bit flipped in each of
    the 32 expected bytes in turn gives 0, with whole neighbours still 1.  A compare that skips a
    word, or a byte order error, fails here."""
    q = LENGTHS.index(64)
    left, right = LENGTHS.index(63), LENGTHS.index(65)
    entries = [(left, 0, 63, 0), (q, 0, 64, 0), (right, 0, 65, 0)]
    flags, ok = _call(reference, entries, None)
    assert list(ok) == [1, 1, 1]
    for byte in range(32):
        def edit(rows, byte=byte):
            rows[1, byte] ^= 1 << (byte % 8)
        flags, ok = _call(reference, entries, None, rows_edit=edit)
        assert list(ok) == [1, 0, 1], byte
    # and through two calls (a 128-byte copy as 64 + 64), the same for the resumed chain
    pool = Pool(1)
    for byte in (0, 3, 4, 15, 16, 28, 31):
        def edit_row(row, byte=byte):
            row[byte] ^= 0x80
        verdict = _through(reference, [LENGTHS.index(128)], 64, pool, rows_edit_at=(0, edit_row))
        assert verdict == {0: 0}, byte


def test_one_call_mixes_first_middle_last_and_whole(reference):
    """300 copies started over three calls, so that one call holds FIRST, middle, LAST and
    FIRST|LAST entries of different copies: more than 256 items (two workgroups), in shuffled
    entry order and with shuffled slots.  One in seven copies is damaged."""
    copies, _ = reference
    S = 64
    n = len(copies)
    rng = np.random.default_rng(11)
    slot = rng.permutation(n)
    pool = Pool(n)
    bad_byte = {q: int(rng.integers(0, len(copies[q]))) for q in range(0, n, 7)}
    # two cycles of the lengths start in the first call, two in the second, the rest in the third,
    # which then holds their later segments beside 244 new copies
    start = lambda q: 0 if q < 28 else 1 if q < 56 else 2  # noqa: E731
    plan = {}
    for q in range(n):
        for r, (off, seg) in enumerate(_segments(len(copies[q]), S)):
            plan.setdefault(start(q) + r, []).append((q, off, seg, int(slot[q])))
    mixed = ended = 0
    for r in sorted(plan):
        entries = [plan[r][k] for k in rng.permutation(len(plan[r]))]
        damage = {k: bad_byte[q] - off for k, (q, off, seg, _) in enumerate(entries)
                  if q in bad_byte and off <= bad_byte[q] < off + seg}
        flags, ok = _call(reference, entries, pool, damage)
        for k, fl in enumerate(flags):
            if fl & L_:
                assert ok[k] == (0 if entries[k][0] in bad_byte else 1), entries[k]
                ended += 1
        if set(flags) == {0, F, L_, F | L_} and len(entries) > 256:
            mixed += 1
    assert mixed >= 1 and ended == n


def test_whole_entries_need_no_pool_and_equal_verify_ragged(reference):
    """A batch of FIRST|LAST entries touches no record (no pool at all) and gives the flags of
    cec_verify_ragged with one chunk per part, damaged copies among them."""
    copies, digests = reference
    entries = [(q, 0, L, 0xFFFFFFFF) for q, L in enumerate(LENGTHS)]  # the slot is ignored
    damage = {2: 0, 5: 64, 9: 128, 13: 319}
    flags, ok = _call(reference, entries, None, damage)
    assert set(flags) == {F | L_}
    region, offs, segs, _, rows, _ = _stage(reference, entries, damage)
    exp = torch.from_numpy(rows).to(DEV)
    want = ce.verify_ragged(1, region.data_ptr() + GUARD, offs, segs, None, exp.data_ptr())
    assert bytes(ok) == want
    assert list(ok) == [0 if k in damage else 1 for k in range(len(entries))]


def test_a_slot_serves_another_copy_right_after_its_last(reference):
    """One state slot: copy A's LAST in one call, copy B's FIRST on the same slot in the next."""
    pool = Pool(1)
    a, b = LENGTHS.index(193), LENGTHS.index(320)
    for q in (a, b, a):
        for off, seg in _segments(LENGTHS[q], 64):
            flags, ok = _call(reference, [(q, off, seg, 0)], pool)
            assert _last_ok(flags, ok) in ([], [1])


def test_calls_queued_back_to_back_on_one_stream(reference):
    """The segments of two copies queued without a wait between the calls: the stream orders
    them.  One of the two copies is damaged in its middle segment."""
    copies, digests = reference
    qa, qb = LENGTHS.index(320), LENGTHS.index(193)
    pool = Pool(2)
    keep, verdicts = [], []
    for r in range(3):  # segments of 128: 320 = 128 + 128 + 64, 193 = 128 + 65
        entries = [(q, *_segments(len(copies[q]), 128)[r], x) for x, q in enumerate((qa, qb))
                   if r < len(_segments(len(copies[q]), 128))]
        region, offs, segs, flags, rows, _ = _stage(reference, entries,
                                                    {0: 7} if r == 1 else None)
        exp = torch.from_numpy(rows).to(DEV)
        okb = torch.full((len(entries),), CANARY, dtype=torch.uint8, device=DEV)
        keep.append((region, exp, okb))
        ce.verify_segments(region.data_ptr() + GUARD, offs, segs, [e[3] for e in entries], flags,
                           pool.ptr, pool.n_slots, exp.data_ptr(), okb.data_ptr())
        verdicts.append((flags, okb))
    torch.cuda.synchronize()
    got = [[int(v) for v in okb.cpu().numpy()] for _, okb in verdicts]
    assert got == [[CANARY, CANARY], [CANARY, 1], [0]]
    assert pool.guards_intact()
