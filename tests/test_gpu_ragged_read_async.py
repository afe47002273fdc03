"""Ragged read without the wait on the GPU: cec_read_ragged_async / cec_resilver_ragged_async,
whose decode plan decode_plan_kernel (csrc/plan_kernels.hip) builds on the device from the
verification's flags.  The planner is tested through its outputs: for every verified set of the
small codes the rebuilt bytes must equal the CPU oracle's chunks, which they do only if the
part's record (inputs, outputs, inverse, table words) is the right one.  Integer work: every
comparison is exact.

As in tests/test_gpu_ragged_read.py the device buffer is filled with 0xA5, only the loaded chunks
are written into it, and the WHOLE buffer is compared with the expected image, so a stray write
(into padding, a verified chunk, a part that cannot be decoded, or behind the last part) shows.
The outputs are page-locked and filled with 0xEE before every call."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import LENGTHS  # noqa: E402
from test_gpu_ragged_read import (CANARY, VERIFIED, _assert_image, _erasures, _image,  # noqa: E402
                                  _loaded, _oracle_parts, _stride)

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda", 0)
FILL = 0xEE
CYCLE = [1, 15, 16, 17, 55, 683]
MODES = pytest.mark.parametrize("resilver", [False, True], ids=["read", "resilver"])


class Case:
    """One batch as it goes up and what must come back: `flags` [n][t] (0, 1 or
    PRESENT_VERIFIED) are the loaded chunks, `flip` lists (k, i) whose first byte goes up
    flipped, `expected` replaces the oracle's digests, `fails` lists the loaded chunks that will
    not verify (default: the flipped ones).  The prediction is the one of
    test_gpu_ragged_read._read: a loaded chunk verifies unless it was flipped (a PRESENT_VERIFIED
    one always); a part with >= d verified chunks has every unverified slot of the mode rebuilt
    over exactly L bytes; a part with fewer has nothing written (its absent slots are
    unspecified and left out of the comparison)."""

    def __init__(self, rs, parts, flags, resilver, flip=(), expected=None, fails=None):
        d, t = rs.data_shard_count(), rs.total_shard_count()
        fails = flip if fails is None else fails
        n = len(parts)
        self.rs, self.parts, self.flags, self.resilver = rs, parts, flags, resilver
        self.n, self.t = n, t
        self.lens = [c.shape[1] for c, _ in parts]
        self.offs, total = ce.ragged_layout(t, self.lens)
        self.up = []
        for k, (chunks, _) in enumerate(parts):
            row = []
            for i in range(t):
                c = chunks[i].copy() if flags[k, i] else None
                if (k, i) in flip:
                    assert c is not None
                    c[0] ^= 0x01
                row.append(c)
            self.up.append(row)
        self.before = _image(parts, self.offs, total, self.up)
        self.want, self.mask = self.before.copy(), np.ones(self.before.size, bool)
        self.want_ver = np.zeros((n, t), np.uint8)
        self.want_st = np.zeros(n, np.int32)
        for k, (chunks, _) in enumerate(parts):
            L = self.lens[k]
            for i in range(t):
                self.want_ver[k, i] = 1 if flags[k, i] and ((k, i) not in fails or
                                                            flags[k, i] == VERIFIED) else 0
            ok = self.want_ver[k].sum() >= d
            self.want_st[k] = ce.OK if ok else ce.TOO_FEW_SHARDS_PRESENT
            for i in range(t):
                at = self.offs[k] + i * _stride(L)
                if ok and not self.want_ver[k, i] and (i < d or resilver):
                    self.want[at:at + L] = chunks[i]
                elif not ok and not flags[k, i]:
                    self.mask[at:at + L] = False
        dig = np.stack([dg for _, dg in parts]) if expected is None else expected
        self.dig = np.ascontiguousarray(dig)

    def upload(self):
        """Device copies of the buffer and the digests, and 0xEE-filled page-locked outputs."""
        self.buf = torch.from_numpy(self.before).to(DEV)
        self.dexp = torch.from_numpy(self.dig).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.ver = ce.HostBuffer(self.n * self.t)
        self.st = ce.HostBuffer(self.n * 4)
        self.ver.array[:] = FILL
        self.st.array[:] = FILL
        torch.cuda.synchronize()
        return self

    def queue(self, stream=None):
        fn = ce.resilver_ragged_async if self.resilver else ce.read_ragged_async
        fn(self.rs, self.buf.data_ptr(), self.offs, self.lens, self.flags.tobytes(),
           self.dexp.data_ptr(), self.ver, self.st, stream)

    def outputs_untouched(self):
        return bool((self.ver.array == FILL).all() and (self.st.array == FILL).all())

    def statuses(self):
        return self.st.array.view(np.int32)

    def check(self):
        """After the stream's work is done."""
        got_ver = self.ver.array.reshape(self.n, self.t)
        bad = np.flatnonzero((got_ver != self.want_ver).any(axis=1))
        assert bad.size == 0, f"verified flags of parts {bad[:8]}: {got_ver[bad[0]]} " \
                              f"want {self.want_ver[bad[0]]}"
        bad = np.flatnonzero(self.statuses() != self.want_st)
        assert bad.size == 0, f"status of parts {bad[:8]}: {self.statuses()[bad[0]]}"
        _assert_image(self.buf.cpu().numpy(), self.want, self.mask)


def _run(rs, parts, flags, resilver, **kw):
    c = Case(rs, parts, flags, resilver, **kw).upload()
    before = ce.ragged_read_stats()
    c.queue()
    torch.cuda.synchronize()
    c.check()
    covered = rs.data_shard_count() <= 32 and rs.parity_shard_count() <= 8
    after = ce.ragged_read_stats()
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if covered else (0, 1))
    return c


# ----------------------------------------------------------------------------------------------
# 1. every verified set of the small codes
# ----------------------------------------------------------------------------------------------

def _every_set(d, p):
    """One row per verified set with >= d chunks (ascending size, lexicographic), then a handful
    with fewer: none, one chunk, d - 1 data chunks, d - 1 chunks from the top."""
    t = d + p
    rows = []
    for size in range(d, t + 1):
        for keep in itertools.combinations(range(t), size):
            row = np.zeros(t, np.uint8)
            row[list(keep)] = 1
            rows.append(row)
    full = len(rows)
    for keep in ([], [t - 1], list(range(d - 1)), list(range(t - d + 1, t)), [0] if d > 1 else []):
        row = np.zeros(t, np.uint8)
        row[keep] = 1
        assert row.sum() < d
        rows.append(row)
    return np.stack(rows), full


@pytest.fixture(scope="module")
def every_set():
    """Per small code: (oracle parts, flags, sets with >= d): computed once, never modified."""
    out = {}
    for (d, p), count in (((3, 2), 16), ((5, 5), 638), ((10, 4), 1471)):
        flags, full = _every_set(d, p)
        assert full == count
        lens = [CYCLE[k % len(CYCLE)] for k in range(len(flags))]
        out[(d, p)] = (_oracle_parts(d, p, lens, 7 * d + p), flags, full)
    return out


@MODES
@pytest.mark.parametrize("d,p", [(3, 2), (5, 5), (10, 4)])
def test_every_verified_set_rebuilds_the_oracles_chunks(d, p, resilver, every_set):
    parts, flags, full = every_set[(d, p)]
    c = _run(ce.ReedSolomon(d, p), parts, flags, resilver)
    st = c.statuses()
    assert (st[:full] == ce.OK).all()
    assert (st[full:] == ce.TOO_FEW_SHARDS_PRESENT).all() and len(st) - full >= 4


# ----------------------------------------------------------------------------------------------
# 2. loaded but damaged
# ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_batches():
    shapes = [(1, 1), (3, 2), (10, 4), (17, 3), (20, 8), (2, 10)]
    return {(d, p): _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in shapes}


@MODES
def test_flipped_byte_with_spare_chunks_is_rebuilt_in_its_own_slot(resilver, oracle_batches):
    d, p = 10, 4
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, d + p, 2, 31)
    flip = set()
    for k in range(0, len(parts), 2):  # a loaded data chunk of some parts, a parity chunk of others
        on = np.flatnonzero(flags[k])
        pick = on[on < d] if k % 4 == 0 else on[on >= d]
        flip.add((k, int(pick[k % len(pick)])))
    assert any(i < d for _, i in flip) and any(i >= d for _, i in flip)
    c = _run(ce.ReedSolomon(d, p), parts, flags, resilver, flip=flip)
    assert (c.statuses() == ce.OK).all()
    assert all(c.ver.array[k * (d + p) + i] == 0 for k, i in flip)


@MODES
def test_flipped_byte_with_exactly_d_loaded_leaves_the_part_short(resilver, oracle_batches):
    d, p = 3, 2
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, d + p, 0, 22)
    flip = {(k, int(np.flatnonzero(flags[k])[k % d])) for k in range(0, len(parts), 3)}
    c = _run(ce.ReedSolomon(d, p), parts, flags, resilver, flip=flip)
    assert [s != ce.OK for s in c.statuses()] == [k % 3 == 0 for k in range(len(parts))]


def test_present_verified_is_trusted(oracle_batches):
    """A PRESENT_VERIFIED chunk with a wrong expected digest is used and reported verified; the
    same chunk flagged 1 fails and, with exactly d loaded, nothing decodes."""
    d, p = 3, 2
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, d + p, 0, 23)
    dig = np.stack([dg for _, dg in parts]).copy()
    trusted = [(k, int(np.flatnonzero(flags[k])[0])) for k in range(len(parts))]
    marked = flags.copy()
    for k, i in trusted:
        dig[k, i] ^= 0xFF
        marked[k, i] = VERIFIED
    rs = ce.ReedSolomon(d, p)
    c = _run(rs, parts, marked, False, expected=dig)
    assert (c.statuses() == ce.OK).all()
    # flagged 1, the wrong digest counts: d - 1 verified, nothing decodes
    c = _run(rs, parts, flags, False, expected=dig, fails=set(trusted))
    assert (c.statuses() == ce.TOO_FEW_SHARDS_PRESENT).all()
    assert all(c.ver.array[k * (d + p) + i] == 0 for k, i in trusted)


# ----------------------------------------------------------------------------------------------
# 3. wide shapes
# ----------------------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("d,p", [(20, 8), (17, 3), (1, 1)])
def test_wide_shapes_with_seeded_erasures(d, p, resilver, oracle_batches):
    parts = oracle_batches[(d, p)]
    t = d + p
    flags = _erasures(len(parts), t, p, 100 * d + p)
    missing = t - flags.sum(axis=1)
    assert set(missing) == set(range(p + 1))
    assert flags[1, :d].all() and not flags[1].all()  # a part that misses only parity
    _run(ce.ReedSolomon(d, p), parts, flags, resilver)


@MODES
def test_one_byte_beside_one_mib_beside_683_bytes(resilver):
    d, p = 10, 4
    parts = _oracle_parts(d, p, [1, 1 << 20, 683], 6)
    flags = np.ones((3, d + p), np.uint8)
    flags[0, [0, 13]] = 0
    flags[1, [2, 5, 9, 11]] = 0
    flags[2, [0, 1, 2]] = 0
    _run(ce.ReedSolomon(d, p), parts, flags, resilver)


# ----------------------------------------------------------------------------------------------
# 4. the same answer as the synchronous call, and as read_batch part by part
# ----------------------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_same_answer_as_the_synchronous_call(d, p, resilver, oracle_batches):
    parts = oracle_batches[(d, p)]
    t = d + p
    rs = ce.ReedSolomon(d, p)
    flags = _loaded(len(parts), d, t, 1, 41)
    flip = {(k, int(np.flatnonzero(flags[k])[k % (d + 1)])) for k in range(0, len(parts), 3)}
    for k in range(1, len(parts), 6):  # and parts left short: d - 1 loaded
        flags[k, np.flatnonzero(flags[k])[:2]] = 0
    c = _run(rs, parts, flags, resilver, flip=flip)
    assert set(c.statuses()) == {ce.OK, ce.TOO_FEW_SHARDS_PRESENT}
    sync_buf = torch.from_numpy(c.before).to(DEV)
    fn = ce.resilver_ragged if resilver else ce.read_ragged
    ver, st = fn(rs, sync_buf.data_ptr(), c.offs, c.lens, flags.tobytes(), c.dexp.data_ptr())
    torch.cuda.synchronize()
    assert ver == c.ver.array.tobytes() and st == list(c.statuses())
    _assert_image(c.buf.cpu().numpy(), sync_buf.cpu().numpy(), c.mask)
    if (d, p) != (10, 4):
        return
    one = ce.resilver_batch if resilver else ce.read_batch
    for k in range(len(parts)):  # the same flags part by part through the uniform form
        x = torch.full((1, t, _stride(c.lens[k])), CANARY, dtype=torch.uint8, device=DEV)
        for i in range(t):
            if c.up[k][i] is not None:
                x[0, i, :c.lens[k]] = torch.from_numpy(c.up[k][i]).to(DEV)
        v1, s1 = one(rs, ce.PartBatch.from_tensor(x, c.lens[k]), flags[k].tobytes(),
                     c.dexp[k].data_ptr())
        assert v1 == ver[k * t:(k + 1) * t] and s1 == [st[k]], k


# ----------------------------------------------------------------------------------------------
# 5. outside the kernel's scope
# ----------------------------------------------------------------------------------------------

@MODES
def test_rs_2_10_takes_the_host_plan_inside_the_call(resilver, oracle_batches):
    d, p = 2, 10
    parts = oracle_batches[(d, p)]
    flags = _erasures(len(parts), d + p, p, 100 * d + p)
    before = ce.ragged_read_stats()
    _run(ce.ReedSolomon(d, p), parts, flags, resilver)  # asserts host_planned + 1 itself
    after = ce.ragged_read_stats()
    assert after[1] == before[1] + 1 and after[0] == before[0]


# ----------------------------------------------------------------------------------------------
# 6, 7. no wait in the call
# ----------------------------------------------------------------------------------------------

CHAIN = 8 << 20  # one SHA-256 lane over 8 MiB: >= ~250 ms of queued work (31-42 ms per MiB)


def _queue_long_chain(chunk, dig, stream):
    """cec_sha256_batch of one 8 MiB chunk on `stream`, and an event behind it."""
    ce.sha256_batch(ce.PartBatch.from_tensor(chunk, CHAIN), 0, 1, dig.data_ptr(), stream)
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _batch_of_25(rs, oracle_batches, seed, resilver=False):
    d, t = rs.data_shard_count(), rs.total_shard_count()
    parts = oracle_batches[(d, t - d)][:25]
    flags = _loaded(25, d, t, 1, seed)
    flip = {(k, int(np.flatnonzero(flags[k])[k % (d + 1)])) for k in range(0, 25, 4)}
    return Case(rs, parts, flags, resilver, flip=flip)


def test_the_call_returns_before_the_streams_earlier_work_is_done(oracle_batches):
    rs = ce.ReedSolomon(10, 4)
    stream = torch.cuda.Stream()
    chunk = torch.zeros((1, 1, CHAIN), dtype=torch.uint8, device=DEV)
    dig = torch.zeros(32, dtype=torch.uint8, device=DEV)
    # first use: the codec's device matrix, the scratch buffers, the kernels' code objects
    warm = _batch_of_25(rs, oracle_batches, 51).upload()
    warm.queue(stream)
    stream.synchronize()
    warm.check()
    c = _batch_of_25(rs, oracle_batches, 52).upload()
    ev = _queue_long_chain(chunk, dig, stream)
    c.queue(stream)
    done, untouched = ev.query(), c.outputs_untouched()
    stream.synchronize()
    assert not done, "the 8 MiB chain in front had completed when the call returned: it waited"
    assert untouched, "an output was written before the stream's work was done"
    c.check()


def test_two_batches_on_two_streams_from_one_thread(oracle_batches):
    rs = ce.ReedSolomon(10, 4)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    chunks = [torch.zeros((1, 1, CHAIN), dtype=torch.uint8, device=DEV) for _ in streams]
    digs = [torch.zeros(32, dtype=torch.uint8, device=DEV) for _ in streams]
    for s in streams:  # first use, as above
        warm = _batch_of_25(rs, oracle_batches, 61).upload()
        warm.queue(s)
        s.synchronize()
    cases = [_batch_of_25(rs, oracle_batches, 62 + q, resilver=q == 1).upload() for q in range(2)]
    evs = [_queue_long_chain(chunks[q], digs[q], streams[q]) for q in range(2)]
    for q in range(2):
        cases[q].queue(streams[q])
    done = [ev.query() for ev in evs]
    untouched = [c.outputs_untouched() for c in cases]
    for s in streams:
        s.synchronize()
    assert done == [False, False], "a call waited for its stream"
    assert untouched == [True, True]
    for c in cases:
        c.check()
