"""Ragged read on the GPU: parts of different chunk lengths rebuilt (cec_reconstruct_ragged),
verified and rebuilt (cec_read_ragged / cec_resilver_ragged) in one launch sequence, and the
host-staged cec_parts_read on top, against the CPU oracle's chunks.  Integer work: every
comparison is exact.

The device buffer is filled with 0xA5 and only the present chunks are written into it, so a
comparison of the WHOLE buffer with the expected image shows every byte the engine wrote: the
rebuilt chunks over exactly L_k bytes, and nothing in the padding up to a stride, between parts,
in a present chunk, in a part that was not listed or behind the last part."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import LENGTHS, SHAPES as WRITE_SHAPES  # noqa: E402
from test_ragged_read import _parts_read_raw  # noqa: E402

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda", 0)
CANARY = 0xA5
SHAPES = WRITE_SHAPES + [(2, 10)]
VERIFIED = ce.PRESENT_VERIFIED


def _stride(L):
    return (L + 15) // 16 * 16


def _oracle_parts(d, p, lens, seed):
    """Per chunk length: (chunks (d+p, L), digests (d+p, 32)) as the CPU oracle stores the part."""
    out = []
    for k, L in enumerate(lens):
        data = gen_bytes(seed * 1000 + k, d * L).reshape(d, L)
        cs, par, dig = oracle.part_encode(d, p, data.reshape(-1), d * L)
        assert cs == L
        out.append((np.concatenate([data, par]), dig))
    return out


@pytest.fixture(scope="module")
def oracle_batches():
    """One batch per shape, one part per chunk length: computed once, shared, never modified."""
    return {(d, p): _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in SHAPES}


def _erasures(n, t, p, seed):
    """Part k misses k % (p+1) chunks, at positions from a seeded permutation: one batch mixes
    every erasure count 0..p.  Part 1 (one chunk missing) draws it among the parity chunks, so
    every batch has a part that misses only parity.  Returns the present flags [n][t]."""
    rng = np.random.default_rng(seed)
    pres = np.ones((n, t), np.uint8)
    for k in range(n):
        pres[k, rng.permutation(t)[:k % (p + 1)]] = 0
    if n > 1:
        pres[1] = 1
        pres[1, t - p + rng.integers(p)] = 0
    return pres


def _image(parts, offs, total, up):
    """The buffer as it goes up: 0xA5 everywhere (64 canary bytes behind the last part), then
    up[k][i] (bytes (L,) or None) at each chunk's place."""
    img = np.full(total + 64, CANARY, np.uint8)
    for k, (chunks, _) in enumerate(parts):
        t, L = chunks.shape
        for i in range(t):
            if up[k][i] is not None:
                at = offs[k] + i * _stride(L)
                img[at:at + L] = up[k][i]
    return img


def _assert_image(got, want, mask=None):
    diff = got != want
    if mask is not None:
        diff &= mask
    if diff.any():
        bad = np.flatnonzero(diff)
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} "
                             f"(got {got[bad[0]]:#x}, want {want[bad[0]]:#x})")


def _reconstruct(rs, parts, pres, data_only, offs=None, total=None):
    """One cec_reconstruct_ragged call; compares the whole buffer with the expected image."""
    d, t = rs.data_shard_count(), rs.total_shard_count()
    lens = [c.shape[1] for c, _ in parts]
    if offs is None:
        offs, total = ce.ragged_layout(t, lens)
    up = [[c[i] if pres[k, i] else None for i in range(t)] for k, (c, _) in enumerate(parts)]
    before = _image(parts, offs, total, up)
    want = before.copy()
    for k, (chunks, _) in enumerate(parts):
        L = lens[k]
        for i in range(t):
            if not pres[k, i] and (i < d or not data_only):
                at = offs[k] + i * _stride(L)
                want[at:at + L] = chunks[i]
    buf = torch.from_numpy(before).to(DEV)
    assert buf.data_ptr() % 16 == 0
    ce.reconstruct_ragged(rs, buf.data_ptr(), offs, lens, pres.tobytes(), data_only)
    torch.cuda.synchronize()
    _assert_image(buf.cpu().numpy(), want)


@pytest.mark.parametrize("data_only", [False, True], ids=["all", "data_only"])
@pytest.mark.parametrize("d,p", SHAPES)
def test_reconstruct_ragged_mixed_erasures(d, p, data_only, oracle_batches):
    parts = oracle_batches[(d, p)]
    t = d + p
    pres = _erasures(len(parts), t, p, 100 * d + p)
    missing = t - pres.sum(axis=1)
    assert set(missing) == set(range(p + 1))
    assert any(pres[k, :d].all() and not pres[k].all() for k in range(len(parts)))  # parity only
    assert (missing == p).any()
    if (d, p) == (2, 10):  # wider than the shared launch's 8 rows: the row-group launches
        assert (missing == 9).any() and (missing == 10).any()
    _reconstruct(ce.ReedSolomon(d, p), parts, pres, data_only)


def test_reconstruct_ragged_spaced_offsets(oracle_batches):
    """Offsets need not be packed: parts with unused space between them."""
    d, p = 3, 2
    parts = oracle_batches[(d, p)][:12]
    offs, total = ce.ragged_layout(d + p, LENGTHS[:12])
    offs = [o + 4096 * k + 16 * (k % 3) for k, o in enumerate(offs)]
    pres = _erasures(12, d + p, p, 7)
    _reconstruct(ce.ReedSolomon(d, p), parts, pres, False, offs, total + 4096 * 12 + 64)


def test_reconstruct_ragged_uniform_equals_reconstruct_batch():
    d, p, n, L = 10, 4, 8, 4096
    t = d + p
    rs = ce.ReedSolomon(d, p)
    data = gen_bytes(78, n * d * L).reshape(n, d, L)
    full = torch.zeros((n, t, L), dtype=torch.uint8, device=DEV)
    full[:, :d] = torch.from_numpy(data).to(DEV)
    ce.encode_batch(rs, ce.PartBatch.from_tensor(full, L))
    pres = _erasures(n, t, p, 9)
    assert len(set(t - pres.sum(axis=1))) == p + 1
    gone = torch.from_numpy(pres == 0).to(DEV)
    for data_only in (False, True):
        a = full.clone()
        a[gone] = CANARY
        b = a.clone()
        ce.reconstruct_batch(rs, ce.PartBatch.from_tensor(a, L), pres.tobytes(), data_only)
        offs, total = ce.ragged_layout(t, [L] * n)
        assert total == n * t * L
        ce.reconstruct_ragged(rs, b.data_ptr(), offs, [L] * n, pres.tobytes(), data_only)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        if not data_only:
            assert torch.equal(b, full)


def test_reconstruct_ragged_4096_one_byte_parts():
    d, p, n = 10, 4, 4096
    t = d + p
    parts = _oracle_parts(d, p, [1] * n, 5)
    pres = np.ones((n, t), np.uint8)
    for k in range(n):  # cycling patterns: k % 5 chunks missing from position k % t on
        for m in range(k % (p + 1)):
            pres[k, (k + 3 * m) % t] = 0
    assert len({row.tobytes() for row in pres}) > 40
    _reconstruct(ce.ReedSolomon(d, p), parts, pres, False)


def test_reconstruct_ragged_one_byte_beside_one_mib():
    d, p = 10, 4
    parts = _oracle_parts(d, p, [1, 1 << 20, 1, 683], 6)
    pres = np.ones((4, d + p), np.uint8)
    pres[0, [0, 13]] = 0
    pres[1, [2, 5, 9, 11]] = 0
    pres[2, [1]] = 0
    pres[3, [0, 1, 2]] = 0
    _reconstruct(ce.ReedSolomon(d, p), parts, pres, False)


# ----------------------------------------------------------------------------------------------
# cec_read_ragged / cec_resilver_ragged
# ----------------------------------------------------------------------------------------------

def _read(rs, parts, flags, resilver, flip=(), expected=None, per_part=False):
    """One cec_read_ragged / cec_resilver_ragged call over `parts` with the loaded chunks of
    `flags` ([n][t]: 0, 1 or PRESENT_VERIFIED); `flip` lists (k, i) whose first byte goes up
    flipped; `expected` replaces the oracle's digests.  Predicts the verified flags and the
    statuses, compares them and the whole buffer (a TOO_FEW part: its loaded chunks as they went
    up, its padding canary, its other slots left out), and returns (verified, status)."""
    d, t = rs.data_shard_count(), rs.total_shard_count()
    n = len(parts)
    lens = [c.shape[1] for c, _ in parts]
    offs, total = ce.ragged_layout(t, lens)
    up = []
    for k, (chunks, _) in enumerate(parts):
        row = []
        for i in range(t):
            c = chunks[i].copy() if flags[k, i] else None
            if (k, i) in flip:
                assert c is not None
                c[0] ^= 0x01
            row.append(c)
        up.append(row)
    before = _image(parts, offs, total, up)
    want, mask = before.copy(), np.ones(before.size, bool)
    want_ver = np.zeros((n, t), np.uint8)
    want_st = []
    for k, (chunks, _) in enumerate(parts):
        L = lens[k]
        for i in range(t):
            want_ver[k, i] = 1 if flags[k, i] and ((k, i) not in flip or
                                                   flags[k, i] == VERIFIED) else 0
        ok = want_ver[k].sum() >= d
        want_st.append(ce.OK if ok else ce.TOO_FEW_SHARDS_PRESENT)
        for i in range(t):
            at = offs[k] + i * _stride(L)
            if ok and not want_ver[k, i] and (i < d or resilver):
                want[at:at + L] = chunks[i]
            elif not ok and not flags[k, i]:
                mask[at:at + L] = False  # unspecified: left out of the comparison
    dig = np.stack([dg for _, dg in parts]) if expected is None else expected
    dexp = torch.from_numpy(np.ascontiguousarray(dig)).to(DEV)
    buf = torch.from_numpy(before).to(DEV)
    fn = ce.resilver_ragged if resilver else ce.read_ragged
    ver, st = fn(rs, buf.data_ptr(), offs, lens, flags.tobytes(), dexp.data_ptr())
    torch.cuda.synchronize()
    assert ver == want_ver.tobytes()
    assert st == want_st
    _assert_image(buf.cpu().numpy(), want, mask)
    if per_part:  # the same flags and bytes part by part through the uniform form
        one = ce.resilver_batch if resilver else ce.read_batch
        for k, (chunks, _) in enumerate(parts):
            x = torch.full((1, t, _stride(lens[k])), CANARY, dtype=torch.uint8, device=DEV)
            for i in range(t):
                if up[k][i] is not None:
                    x[0, i, :lens[k]] = torch.from_numpy(up[k][i]).to(DEV)
            v1, s1 = one(rs, ce.PartBatch.from_tensor(x, lens[k]), flags[k].tobytes(),
                         dexp[k].data_ptr())
            assert v1 == ver[k * t:(k + 1) * t] and s1 == [st[k]], k
    return ver, st


def _loaded(n, d, t, extra, seed):
    """d + extra chunks loaded per part, at seeded positions."""
    rng = np.random.default_rng(seed)
    flags = np.zeros((n, t), np.uint8)
    for k in range(n):
        flags[k, rng.permutation(t)[:min(t, d + extra)]] = 1
    return flags


@pytest.mark.parametrize("resilver", [False, True], ids=["read", "resilver"])
@pytest.mark.parametrize("d,p", [(3, 2), (10, 4), (2, 10)])
def test_read_ragged_all_loaded_chunks_good(d, p, resilver, oracle_batches):
    """d chunks loaded per part, all good: every part decodes; a read leaves missing parity
    alone, a resilver rebuilds it (the expected image of _read has both)."""
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, d + p, 0, 3 * d + p)
    assert any(not flags[k, d:].all() for k in range(len(parts)))  # some parity is missing
    assert any(not flags[k, :d].all() for k in range(len(parts)))  # and some data
    ver, st = _read(ce.ReedSolomon(d, p), parts, flags, resilver, per_part=(d, p) == (10, 4))
    assert st == [ce.OK] * len(parts)


@pytest.mark.parametrize("resilver", [False, True], ids=["read", "resilver"])
def test_read_ragged_flipped_byte_with_spare_chunks(resilver, oracle_batches):
    """More than d chunks loaded, one byte flipped in a loaded chunk of every third part: its
    flag is 0, the part decodes and the chunk is rebuilt from the others."""
    d, p = 10, 4
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, d + p, 1, 21)
    flip = {(k, int(np.flatnonzero(flags[k])[k % (d + 1)])) for k in range(0, len(parts), 3)}
    assert any(i < d for _, i in flip) and any(i >= d for _, i in flip)
    ver, st = _read(ce.ReedSolomon(d, p), parts, flags, resilver, flip=flip, per_part=True)
    assert st == [ce.OK] * len(parts)
    assert all(ver[k * (d + p) + i] == 0 for k, i in flip)


@pytest.mark.parametrize("resilver", [False, True], ids=["read", "resilver"])
def test_read_ragged_flipped_byte_with_exactly_d_loaded(resilver, oracle_batches):
    """Exactly d loaded: a flipped byte leaves the part short.  TOO_FEW_SHARDS_PRESENT, its
    loaded chunks byte-identical to what went up, padding and gaps canary; the other parts of the
    call decode."""
    d, p = 3, 2
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, d + p, 0, 22)
    flip = {(k, int(np.flatnonzero(flags[k])[k % d])) for k in range(0, len(parts), 3)}
    ver, st = _read(ce.ReedSolomon(d, p), parts, flags, resilver, flip=flip, per_part=True)
    assert [s != ce.OK for s in st] == [k % 3 == 0 for k in range(len(parts))]


def test_read_ragged_present_verified_is_trusted(oracle_batches):
    """A PRESENT_VERIFIED chunk is not hashed: with a wrong expected digest it is still used and
    reported verified; the same chunk flagged 1 fails."""
    d, p = 3, 2
    t = d + p
    parts = oracle_batches[(d, p)]
    flags = _loaded(len(parts), d, t, 0, 23)
    dig = np.stack([dg for _, dg in parts]).copy()
    trusted = [(k, int(np.flatnonzero(flags[k])[0])) for k in range(len(parts))]
    for k, i in trusted:
        dig[k, i] ^= 0xFF
    marked = flags.copy()
    for k, i in trusted:
        marked[k, i] = VERIFIED
    rs = ce.ReedSolomon(d, p)
    ver, st = _read(rs, parts, marked, False, expected=dig)
    assert st == [ce.OK] * len(parts) and all(ver[k * t + i] == 1 for k, i in trusted)
    # flagged 1, the wrong digest counts: d - 1 verified, nothing decodes
    lens = [c.shape[1] for c, _ in parts]
    offs, total = ce.ragged_layout(t, lens)
    up = [[c[i] if flags[k, i] else None for i in range(t)] for k, (c, _) in enumerate(parts)]
    buf = torch.from_numpy(_image(parts, offs, total, up)).to(DEV)
    dexp = torch.from_numpy(dig).to(DEV)
    ver, st = ce.read_ragged(rs, buf.data_ptr(), offs, lens, flags.tobytes(), dexp.data_ptr())
    assert st == [ce.TOO_FEW_SHARDS_PRESENT] * len(parts)
    assert all(ver[k * t + i] == 0 for k, i in trusted)


# ----------------------------------------------------------------------------------------------
# cec_parts_read (host staged)
# ----------------------------------------------------------------------------------------------

FILL = 0xEE


def _file_parts(d, p, sizes, seed):
    """Parts of these byte sizes as the oracle stores them: (chunks (d+p, L), digests)."""
    out = []
    for k, size in enumerate(sizes):
        buf = gen_bytes(seed + k, size)
        cs, par, dig = oracle.part_encode(d, p, buf, size)
        data = np.zeros(d * cs, np.uint8)
        data[:size] = buf
        out.append((np.concatenate([data.reshape(d, cs), par]), dig))
    return out


def _parts_read(rs, parts, flags, data_only, flip=()):
    """Raw cec_parts_read: every slot is caller memory filled with 0xEE, loaded chunks copied in.
    Checks the outputs against the prediction (filled slots equal the oracle's chunks, every
    other slot keeps what it held) and returns (slot bytes [n][t], verified, status)."""
    d, t = rs.data_shard_count(), rs.total_shard_count()
    n = len(parts)
    lens = [c.shape[1] for c, _ in parts]
    slots, held = [], []
    for k, (chunks, _) in enumerate(parts):
        for i in range(t):
            s = (ctypes.c_uint8 * lens[k])()
            if flags[k, i]:
                c = chunks[i].copy()
                if (k, i) in flip:
                    c[-1] ^= 0x80
                ctypes.memmove(s, c.tobytes(), lens[k])
            else:
                ctypes.memset(s, FILL, lens[k])
            slots.append(s)
            held.append(bytes(s))
    ptrs = (ce._u8p * (n * t))(*[ctypes.cast(s, ce._u8p) for s in slots])
    expected = np.ascontiguousarray(np.stack([dg for _, dg in parts])).tobytes()
    verified = (ctypes.c_uint8 * (n * t))()
    status = (ctypes.c_int * n)()
    code = ce._lib.cec_parts_read(
        rs.handle, ptrs, (ctypes.c_size_t * n)(*lens), n,
        ctypes.cast(ctypes.c_char_p(flags.tobytes()), ce._u8p),
        ctypes.cast(ctypes.c_char_p(expected), ce._u8p), 1 if data_only else 0, verified, status)
    assert code == ce.OK, ce.last_error() if hasattr(ce, "last_error") else code
    got = [bytes(s) for s in slots]
    for k, (chunks, _) in enumerate(parts):
        ver = [1 if flags[k, i] and (k, i) not in flip else 0 for i in range(t)]
        assert list(verified[k * t:(k + 1) * t]) == ver, k
        ok = sum(ver) >= d
        assert status[k] == (ce.OK if ok else ce.TOO_FEW_SHARDS_PRESENT), k
        for i in range(t):
            if ok and not ver[i] and (i < d or not data_only):
                assert got[k * t + i] == chunks[i].tobytes(), (k, i, "rebuilt")
            else:
                assert got[k * t + i] == held[k * t + i], (k, i, "untouched")
    return got, bytes(verified), list(status)


def _encode_sizes(d):
    L = 4096
    return [1, 2, 7, 20480, 699051 * 3, d * L, d * L - (d - 1)]


@pytest.mark.parametrize("data_only", [True, False], ids=["read", "resilver"])
@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_parts_read_fills_the_missing_slots(d, p, data_only):
    rs = ce.ReedSolomon(d, p)
    t = d + p
    parts = _file_parts(d, p, _encode_sizes(d), 40)
    flags = np.ones((len(parts), t), np.uint8)
    for k in range(len(parts)):  # one data chunk and, for every other part, one parity chunk
        flags[k, k % d] = 0
        if k % 2:
            flags[k, d + k % p] = 0
    # a loaded chunk that fails verification counts as missing: rebuilt into its own slot
    flip = {(1, (1 % d + 1) % d), (4, d + 1)}
    assert all(flags[k, i] for k, i in flip)
    _parts_read(rs, parts, flags, data_only, flip=flip)


def test_parts_read_python_wrapper():
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    parts = _file_parts(d, p, [1, 683, 20480], 50)
    given, expected = [], []
    for k, (chunks, dig) in enumerate(parts):
        row = [chunks[i].tobytes() for i in range(d + p)]
        row[k % d] = None
        row[d] = (row[d], VERIFIED)
        row[d + 1] = None
        given.append(row)
        expected.append([dig[i].tobytes() for i in range(d + p)])
    out, ver, st = ce.parts_read(rs, given, expected)
    assert st == [ce.OK] * 3
    for k, (chunks, _) in enumerate(parts):
        assert out[k][:d + 1] == [chunks[i].tobytes() for i in range(d + 1)]
        assert out[k][d + 1] is None  # a read never fills parity
    out, ver, st = ce.parts_read(rs, given, expected, data_only=False)
    for k, (chunks, _) in enumerate(parts):
        assert out[k] == [chunks[i].tobytes() for i in range(d + p)]


def test_parts_read_rounds(knob_env):
    """A 1 MiB cap cuts about 3 MiB of parts plus one 2 MiB part into several rounds (the large
    part alone); the results are the same."""
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    sizes = [200_001, 350_017, 1, 2 << 20, 420_000, 683, 510_003, 99_999, 640_000, 333_333,
             250_000, 300_000]
    assert 3_000_000 < sum(sizes) - (2 << 20) < 3_500_000 and max(sizes) > 1 << 20
    parts = _file_parts(d, p, sizes, 60)
    flags = np.ones((len(parts), d + p), np.uint8)
    for k in range(len(parts)):
        flags[k, (k + 1) % (d + p)] = 0
        flags[k, k % d] = 0
    flip = {(9, 1)}  # part 9 misses one chunk: still decodable with this one failing
    assert flags[9].sum() == d + p - 1 and flags[9, 1]
    want = _parts_read(rs, parts, flags, False, flip=flip)
    knob_env.set("CEC_COALESCE_MAX_MIB", "1")
    got = _parts_read(rs, parts, flags, False, flip=flip)
    assert got == want


def test_parts_read_four_threads():
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    jobs = [_file_parts(d, p, [1 + w, 4097 * (w + 1), 70_001, 683, 20480 + w], 100 * w)
            for w in range(4)]
    errors = []

    def work(w):
        try:
            flags = np.ones((5, d + p), np.uint8)
            for k in range(5):
                flags[k, (k + w) % d] = 0
                flags[k, d + (k + w) % p] = 0
            _parts_read(rs, jobs[w], flags, w % 2 == 0)
        except BaseException as e:  # noqa: BLE001  (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,)) for w in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_parts_read_zero_length_in_the_middle():
    rs = ce.ReedSolomon(3, 2)
    present = [0, 1, 1, 1, 1] * 3
    code, untouched = _parts_read_raw(rs, [100, 0, 1000], present)
    assert code == ce.EMPTY_SHARD and untouched
    # well formed: runs (the 0xEE chunks fail verification, so every part is short)
    code, untouched = _parts_read_raw(rs, [100, 1, 1000], present)
    assert code == ce.OK and not untouched
