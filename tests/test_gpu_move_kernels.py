"""move_chunks_kernel and carry_copy_kernel / carry_assign_kernel (csrc/move_kernels.hip) through
the read pipeline's public API, at the shapes that reach each of their branches: the second
half of the unrolled 16-byte load/store pair, a second pass of the outer loop, more than one
256 KiB slice per chunk (vector and byte builds, with a short last slice), the grid-stride loop
past 2048 work items, the packed_ids form (a retry's consume from the carry pool) at chunk
strides above 4 KiB, and the stash's scan with more than one part per thread.

The reference is the stored numpy bytes: data from a seeded generator, parity from
oracle.encode_sep, digests from hashlib.sha256.  Every assertion is bit-exact, and every part
holds different bytes, so a chunk placed at the wrong position cannot pass.  A verified chunk
proves that all L bytes the kernel moved hash to the stored digest.

Branches that cannot be reached through the API, and so have no test here or anywhere:
  * to_batch = 0, the gather direction of move_chunks_kernel: no caller passes it;
  * the byte build of carry_copy_kernel: the pool stride cs is always a multiple of 256 and
    both buffers come from hipMalloc, so the 16-byte build is always taken."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import chunky_ec as ce  # noqa: E402
import oracle  # noqa: E402
from _gen import gen_bytes  # noqa: E402

SLICE = 262144  # kMoveSlice: bytes of a chunk one work item moves
OK, TOO_FEW = ce.OK, ce.TOO_FEW_SHARDS_PRESENT
RP = ce.ReadPipeline


@functools.lru_cache(maxsize=4)
def _store(n, d, p, L, seed):
    """n stored parts of RS(d, p) with chunk length L: ([n][d+p][L] chunks, [n][d+p][32]
    digests), read-only and shared between the tests that ask for the same store."""
    chunks = np.zeros((n, d + p, L), np.uint8)
    dig = np.zeros((n, d + p, 32), np.uint8)
    for k in range(n):
        data = gen_bytes(seed * 1000003 + k, d * L).reshape(d, L)
        st, par = oracle.encode_sep(d, p, list(data))
        assert st == 0
        chunks[k, :d], chunks[k, d:] = data, np.stack(par)
        for i in range(d + p):
            dig[k, i] = np.frombuffer(hashlib.sha256(chunks[k, i].tobytes()).digest(), np.uint8)
    chunks.setflags(write=False)
    dig.setflags(write=False)
    return chunks, dig


def _parts_bytes(rp, slot, n_parts, which):
    """part_bytes of the parts in `which`, from one data_chunks call."""
    ptrs = rp.data_chunks(slot, n_parts)
    return {k: b"".join(ctypes.string_at(int(a), rp.L) for a in ptrs[k]) for k in which}


# --------------------------------------------------------------------------------------------
# a. Packed placement: move_chunks_kernel, to_batch = 1, no packed_ids
# --------------------------------------------------------------------------------------------

ALL, SOME, ONE_BAD, TOO_FEW_LOADED = range(4)


def _packed_batch(rp, d, p, L, parts, seed, kinds, edge):
    """One packed batch through slot 0 of `rp`, asserted in full.  kinds[k] is part k's loaded
    set: all t chunks; a random d of t; d + 1 with one damaged; d - 1 (undecodable).  edge =
    (part, chunk, offset): one more bit flipped, in a loaded chunk of a part that still decodes."""
    t = d + p
    chunks, dig = _store(parts, d, p, L, seed)
    rng = np.random.default_rng(seed)
    present = np.zeros((parts, t), np.uint8)
    flips = {}  # (part, chunk) -> offset of the flipped bit
    for k in range(parts):
        count = {ALL: t, SOME: d, ONE_BAD: d + 1, TOO_FEW_LOADED: d - 1}[kinds[k]]
        loaded = np.sort(rng.choice(t, size=count, replace=False))
        present[k, loaded] = 1
        if kinds[k] == ONE_BAD:
            flips[(k, int(rng.choice(loaded)))] = int(rng.integers(L))
    ek, ei, eoff = edge
    assert kinds[ek] == ALL and (ek, ei) not in flips and 0 <= eoff < L
    flips[(ek, ei)] = eoff
    where = [(k, i) for k in range(parts) for i in range(t) if present[k, i]]
    packed = np.concatenate([chunks[k, i] for k, i in where])
    for j, ki in enumerate(where):
        if ki in flips:
            packed[j * L + flips[ki]] ^= 0x04
    slot, _, _, _ = rp.acquire()
    assert slot == 0
    rp.submit_packed(slot, packed, present, dig.copy(), parts)
    _, ver, st = rp.wait(slot)
    want_st = [TOO_FEW if kinds[k] == TOO_FEW_LOADED else OK for k in range(parts)]
    assert list(st) == want_st
    want_ver = present.copy()
    for k, i in flips:
        want_ver[k, i] = 0
    bad = np.argwhere(ver != want_ver)
    assert len(bad) == 0, f"verified flags differ at (part, chunk) {bad.tolist()}"
    assert ver[ek, ei] == 0  # the flipped bit at the edge offset reached the hash
    good = [k for k in range(parts) if want_st[k] == OK]
    for k, out in _parts_bytes(rp, slot, parts, good).items():
        assert out == chunks[k, :d].tobytes(), f"part {k}"


# L, edge offset: the first byte (or the last one) that only the newly reached branch moves
PACKED_CASES = [
    pytest.param(4096 + 16, 4096, id="n16=257"),        # one lane takes the second half
    pytest.param(8192 - 16, 8192 - 16 - 1, id="n16=511"),   # all lanes but one take it
    pytest.param(8192 + 16, 8192, id="n16=513"),        # the outer loop runs a second time
    pytest.param(SLICE, SLICE - 1, id="slice"),         # exactly one full slice, cs == L
    pytest.param(SLICE + 16, SLICE, id="slice+16"),     # two slices, the last a single word
    pytest.param(2 * SLICE, SLICE, id="2slices"),       # two full slices, cs == L
    pytest.param(SLICE + 1, SLICE, id="slice+1"),       # byte build, the second slice one byte
    pytest.param(3 * SLICE - 5, 2 * SLICE, id="3slices-5"),  # byte build, three slices
]


@pytest.mark.parametrize("flags", [0, RP.REBUILT_ONLY], ids=["full", "rebuilt_only"])
@pytest.mark.parametrize("L,edge_off", PACKED_CASES)
def test_packed_placement_by_chunk_length(L, edge_off, flags):
    """RS(3,2): two batches of different bytes and different loaded sets through the single
    slot, so what the first one left in the device buffer can never satisfy the second.
    flags = 0: every data chunk comes back from the device buffer, so part_bytes compares the
    moved bytes themselves; REBUILT_ONLY: the pointer contract (loaded chunks stay where read)
    at these sizes."""
    d, p = 3, 2
    parts = 5 if L < SLICE else 4
    rp = RP(ce.ReedSolomon(d, p), L, parts, 1, flags)
    for b in range(2):
        kinds = [(k + b) % 4 for k in range(parts)]
        _packed_batch(rp, d, p, L, parts, 50 + b, kinds, (kinds.index(ALL), (1 + 3 * b) % 5,
                                                          edge_off))


@pytest.mark.parametrize("flags", [0, RP.REBUILT_ONLY], ids=["full", "rebuilt_only"])
@pytest.mark.parametrize("d,p,parts,L", [(10, 4, 160, 64), (3, 2, 700, 683)],
                         ids=["2240x64-vector", "3500x683-byte"])
def test_packed_placement_past_the_grid(d, p, parts, L, flags):
    """More than 2048 chunks in one batch, all loaded: the work items past kMoveGrid come from
    the grid-stride loop's second pass.  The flipped bit is in the batch's last chunk."""
    rp = RP(ce.ReedSolomon(d, p), L, parts, 1, flags)
    for b in range(2):
        _packed_batch(rp, d, p, L, parts, 60 + b, [ALL] * parts, (parts - 1, d + p - 1 - b, L - 1))


# --------------------------------------------------------------------------------------------
# b. Carry stash and consume: carry_assign_kernel, carry_copy_kernel, move_chunks_kernel with
#    packed_ids
# --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [SLICE + 16, 8192 + 16], ids=["two-slice-stride", "medium"])
def test_carry_stash_and_consume_by_pool_stride(L):
    """RS(3,2), 4 parts, 2 of them kept (0 < verified < d).  L = 262144 + 16: the pool stride cs
    = 262400 is two slices, the second 256 bytes long and holding the chunk's last 16 bytes;
    L = 8192 + 16: the consume's move runs its outer loop twice.  The retry puts the kept parts
    at other batch positions of the same slot, with the slot bytes of the kept chunks garbage:
    their bytes can only come from the pool."""
    d, p, n = 3, 2, 4
    chunks, dig = _store(n, d, p, L, 70)
    rp = RP(ce.ReedSolomon(d, p), L, n, 1, RP.REBUILT_ONLY | RP.CARRY)
    slot, ch, pres, exp = rp.acquire()
    pres[:] = 0
    pres[0, :] = 1            # decodes
    pres[1, [0, 1, 2]] = 1    # chunk 1 damaged: chunks 0 and 2 kept
    pres[2, [1, 2, 4]] = 1    # decodes (chunk 0 rebuilt)
    pres[3, [0, 3, 4]] = 1    # chunk 3 damaged in its last byte: chunks 0 and 4 kept
    ch[:] = chunks
    ch[1, 1, L // 2] ^= 0x20
    ch[3, 3, L - 1] ^= 0x01
    exp[:] = dig
    rp.submit(slot, n)
    _, ver, st = rp.wait(slot)
    assert list(st) == [OK, TOO_FEW, OK, TOO_FEW]
    assert ver.tolist() == [[1, 1, 1, 1, 1], [1, 0, 1, 0, 0], [0, 1, 1, 0, 1], [1, 0, 0, 0, 1]]
    for k, out in _parts_bytes(rp, slot, n, [0, 2]).items():
        assert out == chunks[k, :d].tobytes(), f"part {k}"
    ids = rp.carry_ids(slot, n)
    assert ids[0] == -1 and ids[2] == -1 and ids[1] >= 0 and ids[3] >= 0 and ids[1] != ids[3]
    # the retry: part 3 at position 0, part 1 at position 1
    slot, ch, pres, exp = rp.acquire()
    pres[:] = 0
    ch[:] = 0x5A
    pres[0, [0, 4]] = ce.PRESENT_VERIFIED
    pres[0, 2] = 1
    ch[0, 2] = chunks[3, 2]
    pres[1, [0, 2]] = ce.PRESENT_VERIFIED
    pres[1, 3] = 1
    ch[1, 3] = chunks[1, 3]
    exp[0], exp[1] = dig[3], dig[1]
    rp.submit_carried(slot, 2, np.array([ids[3], ids[1]], np.int32))
    _, ver, st = rp.wait(slot)
    assert list(st) == [OK, OK]
    assert ver.tolist() == [[1, 0, 1, 0, 1], [1, 0, 1, 1, 0]]
    out = _parts_bytes(rp, slot, 2, [0, 1])
    assert out[0] == chunks[3, :d].tobytes()
    assert out[1] == chunks[1, :d].tobytes()


def test_carry_stash_with_more_parts_than_scan_threads():
    """RS(2,1), L = 16, 1100 parts: carry_assign_kernel's 1024 threads own two parts each, so the
    scan sums real counts across threads, and carry_copy_kernel has 3300 work items.  Part k is
    of kind k % 3: 0 decodes; 1 has chunks 0 and 2 loaded with chunk 0 damaged (one verified of
    the two needed: kept); 2 has one chunk loaded, damaged (nothing to keep).  367 parts are
    kept and the reservation is min(P, max(8, P / 4)) = 275 entries, so exactly the first 275
    kept parts in part order get an id.

    The ids must rise with the part index.  That rests on two things: carry_stash() reserves
    from a FIFO free list that starts as 0, 1, 2, ... on a fresh pipeline, and the kernel hands
    the reserved entries out in part order (each kept part's rank among the kept ones).

    The retry carries those 275 (slot bytes of the kept chunk garbage) and sends the verified
    chunk of the other 92 again; all 367 decode to the stored bytes."""
    d, p, L, n = 2, 1, 16, 1100
    t = d + p
    chunks, dig = _store(n, d, p, L, 80)
    kept = [k for k in range(n) if k % 3 == 1]
    assert len(kept) == 367
    # every kept chunk differs from part to part: an entry filled from the wrong part shows
    assert len({chunks[k, 2].tobytes() for k in kept}) == len(kept)
    rp = RP(ce.ReedSolomon(d, p), L, n, 1, RP.REBUILT_ONLY | RP.CARRY)
    slot, ch, pres, exp = rp.acquire()
    pres[:] = 0
    ch[:] = chunks
    exp[:] = dig
    want_ver = np.zeros((n, t), np.uint8)
    for k in range(n):
        if k % 3 == 0:
            pres[k, :] = 1
            want_ver[k, :] = 1
        elif k % 3 == 1:
            pres[k, [0, 2]] = 1
            ch[k, 0, k % L] ^= 0x80
            want_ver[k, 2] = 1
        else:
            pres[k, 1] = 1
            ch[k, 1, k % L] ^= 0x02
    rp.submit(slot, n)
    _, ver, st = rp.wait(slot)
    assert list(st) == [OK if k % 3 == 0 else TOO_FEW for k in range(n)]
    assert np.array_equal(ver, want_ver)
    whole = list(range(0, n, 3))
    for k, out in _parts_bytes(rp, slot, n, whole).items():
        assert out == chunks[k, :d].tobytes(), f"part {k}"
    ids = rp.carry_ids(slot, n).copy()
    with_id = [k for k in range(n) if ids[k] >= 0]
    assert with_id == kept[:275]
    assert np.all(np.delete(ids, with_id) == -1)
    got = ids[with_id]
    assert len(set(got.tolist())) == 275 and got.min() >= 0
    assert np.all(np.diff(got) > 0), "ids do not rise with the part index"
    # the retry: kept part number r at batch position r
    m = len(kept)
    slot, ch, pres, exp = rp.acquire()
    pres[:] = 0
    ch[:] = 0x5A
    for r, k in enumerate(kept):
        pres[r, 2] = ce.PRESENT_VERIFIED
        if ids[k] < 0:  # no entry: the verified chunk goes up again from the slot
            ch[r, 2] = chunks[k, 2]
        pres[r, 1] = 1
        ch[r, 1] = chunks[k, 1]
        exp[r] = dig[k]
    rp.submit_carried(slot, m, ids[kept])
    _, ver, st = rp.wait(slot)
    assert list(st) == [OK] * m
    assert np.array_equal(ver, np.tile(np.array([0, 1, 1], np.uint8), (m, 1)))
    for r, out in _parts_bytes(rp, slot, m, range(m)).items():
        assert out == chunks[kept[r], :d].tobytes(), f"part {kept[r]} (retry position {r})"
