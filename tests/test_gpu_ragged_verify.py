"""Ragged verify on the GPU: the chunks of parts of different chunk lengths hashed and compared
in one launch (cec_verify_ragged), and the host-staged cec_parts_verify on top, against the CPU
oracle's digests and hashlib.  Integer work: every comparison is exact.

The device buffer is filled with 0xA5, the loaded chunks are written into it, and the WHOLE buffer
is compared before and after every call: a verification writes not one byte of it."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import LENGTHS  # noqa: E402
from test_ragged_verify import _parts_verify_raw  # noqa: E402

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda", 0)
CANARY = 0xA5
SHAPES = [(3, 2), (10, 4), (2, 10)]
VERIFIED = ce.PRESENT_VERIFIED
assert {55, 56, 63, 64, 65, 119, 120} <= set(LENGTHS)  # SHA-256's block and padding edges


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


def _flat_parts(lens, seed):
    """total_shards = 1: independent buffers, digests from hashlib."""
    out = []
    for k, L in enumerate(lens):
        buf = gen_bytes(seed * 1000 + k, L).reshape(1, L)
        dig = np.frombuffer(hashlib.sha256(buf.tobytes()).digest(), np.uint8).reshape(1, 32)
        out.append((buf, dig))
    return out


@pytest.fixture(scope="module")
def batches():
    """One batch per total_shards, one part per chunk length: computed once, shared, never
    modified."""
    out = {d + p: _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in SHAPES}
    out[1] = _flat_parts(LENGTHS, 77)
    return out


def _verify(parts, flags, flip=(), expected=None, offs=None, total=None):
    """One cec_verify_ragged call over `parts` with the loaded chunks of `flags` ([n][t]: 0, 1 or
    PRESENT_VERIFIED; None: a NULL pointer, every chunk loaded); `flip` maps (k, i) to the byte
    index whose low bit goes up flipped; `expected` replaces the parts' digests.  Compares the
    whole buffer before and after, and returns the flags [n][t]."""
    n, t = len(parts), parts[0][0].shape[0]
    lens = [c.shape[1] for c, _ in parts]
    if offs is None:
        offs, total = ce.ragged_layout(t, lens)
    before = np.full(total + 64, CANARY, np.uint8)  # 64 canary bytes behind the last part
    for k, (chunks, _) in enumerate(parts):
        for i in range(t):
            if flags is not None and not flags[k, i]:
                continue
            c = chunks[i].copy()
            if (k, i) in flip:
                c[flip[(k, i)]] ^= 0x01
            at = offs[k] + i * _stride(lens[k])
            before[at:at + lens[k]] = c
    dig = np.stack([dg for _, dg in parts]) if expected is None else expected
    dexp = torch.from_numpy(np.ascontiguousarray(dig)).to(DEV)
    buf = torch.from_numpy(before).to(DEV)
    assert buf.data_ptr() % 16 == 0
    ver = ce.verify_ragged(t, buf.data_ptr(), offs, lens,
                           None if flags is None else flags.tobytes(), dexp.data_ptr())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if not np.array_equal(got, before):
        bad = np.flatnonzero(got != before)
        raise AssertionError(f"{bad.size} bytes written, first at {bad[0]}")
    return np.frombuffer(ver, np.uint8).reshape(n, t)


def _flag_mix(n, t, seed):
    """Every flag kind in one batch: each chunk 0, 1 or PRESENT_VERIFIED from a seeded draw."""
    rng = np.random.default_rng(seed)
    flags = rng.choice(np.array([0, 1, 1, VERIFIED], np.uint8), size=(n, t))
    flags[0, 0], flags[-1, -1], flags[n // 2, t // 2] = 1, 0, VERIFIED
    return flags


@pytest.mark.parametrize("t", [1, 5, 14, 12])
def test_verify_ragged_flag_mix_and_flipped_bits(t, batches):
    """Every flag kind; a bit flipped in the first or the last byte of every third hashed chunk:
    a hashed chunk reports 1 iff it went up intact, a trusted one 1, an absent one 0."""
    parts = batches[t]
    n = len(parts)
    flags = _flag_mix(n, t, 31 * t)
    hashed = [(k, i) for k in range(n) for i in range(t) if flags[k, i] == 1]
    flip = {}
    for x, (k, i) in enumerate(hashed[::3]):
        flip[(k, i)] = 0 if x % 2 == 0 else parts[k][0].shape[1] - 1
    assert len(flip) >= 2 and {0} < set(flip.values())
    want = np.zeros((n, t), np.uint8)
    for k in range(n):
        for i in range(t):
            want[k, i] = 1 if flags[k, i] == VERIFIED or (flags[k, i] and (k, i) not in flip) else 0
    assert {0, 1} == set(want[flags == 1]) and (want[flags == VERIFIED] == 1).all()
    assert np.array_equal(_verify(parts, flags, flip=flip), want)


@pytest.mark.parametrize("t", [1, 5, 14, 12])
def test_verify_ragged_present_null_hashes_every_chunk(t, batches):
    parts = batches[t]
    n = len(parts)
    assert _verify(parts, None).all()
    flip = {(k, (3 * k) % t): (0 if k % 2 else parts[k][0].shape[1] - 1) for k in range(0, n, 2)}
    want = np.ones((n, t), np.uint8)
    for k, i in flip:
        want[k, i] = 0
    assert np.array_equal(_verify(parts, None, flip=flip), want)
    # the same through explicit flags
    assert np.array_equal(_verify(parts, np.ones((n, t), np.uint8), flip=flip), want)


def test_verify_ragged_present_verified_is_trusted(batches):
    """A PRESENT_VERIFIED chunk is not hashed: with a wrong expected digest it still reports 1;
    the same chunk flagged 1 reports 0."""
    t = 5
    parts = batches[t]
    n = len(parts)
    dig = np.stack([dg for _, dg in parts]).copy()
    trusted = [(k, k % t) for k in range(n)]
    for k, i in trusted:
        dig[k, i] ^= 0xFF
    marked = np.ones((n, t), np.uint8)
    for k, i in trusted:
        marked[k, i] = VERIFIED
    assert _verify(parts, marked, expected=dig).all()
    ver = _verify(parts, np.ones((n, t), np.uint8), expected=dig)
    want = np.ones((n, t), np.uint8)
    for k, i in trusted:
        want[k, i] = 0
    assert np.array_equal(ver, want)


def test_verify_ragged_spaced_offsets(batches):
    """Offsets need not be packed: parts with unused space between them."""
    t = 5
    parts = batches[t][:12]
    offs, total = ce.ragged_layout(t, LENGTHS[:12])
    offs = [o + 4096 * k + 16 * (k % 3) for k, o in enumerate(offs)]
    flags = _flag_mix(12, t, 8)
    flip = {(3, 1): 0, (7, 4): LENGTHS[7] - 1}
    flags[3, 1] = flags[7, 4] = 1
    want = (flags != 0).astype(np.uint8)
    want[3, 1] = want[7, 4] = 0
    ver = _verify(parts, flags, flip=flip, offs=offs, total=total + 4096 * 12 + 64)
    assert np.array_equal(ver, want)


def test_verify_ragged_uniform_equals_verify_batch():
    d, p, n, L = 10, 4, 8, 4096
    t = d + p
    rs = ce.ReedSolomon(d, p)
    full = torch.zeros((n, t, L), dtype=torch.uint8, device=DEV)
    full[:, :d] = torch.from_numpy(gen_bytes(79, n * d * L).reshape(n, d, L)).to(DEV)
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device=DEV)
    batch = ce.PartBatch.from_tensor(full, L)
    ce.encode_hash_batch(rs, batch, dig.data_ptr())
    torch.cuda.synchronize()
    full[1, 3, 0] ^= 1
    full[5, 13, L - 1] ^= 1
    pres = np.ones((n, t), np.uint8)
    pres[2, 4] = pres[6, 0] = pres[7, 13] = 0
    dpres = torch.from_numpy(pres).to(DEV)
    ok = torch.full((n, t), 7, dtype=torch.uint8, device=DEV)
    ce.verify_batch(batch, 0, t, dig.data_ptr(), ok.data_ptr(), dpres.data_ptr())
    torch.cuda.synchronize()
    offs, total = ce.ragged_layout(t, [L] * n)
    assert total == n * t * L
    ver = ce.verify_ragged(t, full.data_ptr(), offs, [L] * n, pres.tobytes(), dig.data_ptr())
    want = pres.copy()
    want[1, 3] = want[5, 13] = 0
    assert ver == ok.cpu().numpy().tobytes() == want.tobytes()


def test_verify_ragged_one_byte_beside_one_mib():
    parts = _oracle_parts(10, 4, [1, 1 << 20], 6)
    flags = np.ones((2, 14), np.uint8)
    flags[0, 5], flags[1, 2] = 0, VERIFIED
    flip = {(0, 0): 0, (1, 7): (1 << 20) - 1, (1, 13): 0}
    want = np.ones((2, 14), np.uint8)
    want[0, 5] = want[0, 0] = want[1, 7] = want[1, 13] = 0
    assert np.array_equal(_verify(parts, flags, flip=flip), want)


def test_verify_ragged_4096_one_byte_parts():
    n = 4096
    parts = _flat_parts([1] * n, 5)
    flags = np.ones((n, 1), np.uint8)
    flags[::7] = 0
    flags[3::7] = VERIFIED
    flip = {(k, 0): 0 for k in range(1, n, 5) if flags[k, 0] == 1}
    want = (flags != 0).astype(np.uint8)
    for k, i in flip:
        want[k, i] = 0
    assert len(flip) > 500
    assert np.array_equal(_verify(parts, flags, flip=flip), want)
    # and as RS(3,2) parts: 4096 parts of five one-byte chunks, every chunk hashed
    parts = _oracle_parts(3, 2, [1] * n, 9)
    flip = {(k, k % 5): 0 for k in range(0, n, 3)}
    want = np.ones((n, 5), np.uint8)
    for k, i in flip:
        want[k, i] = 0
    assert np.array_equal(_verify(parts, None, flip=flip), want)


# ----------------------------------------------------------------------------------------------
# cec_parts_verify (host staged)
# ----------------------------------------------------------------------------------------------

PV_LENGTHS = [1, 2, 7, 683, 20480, 65537, (2 << 20) + 1]


@pytest.fixture(scope="module")
def copies():
    """(good copy, its digest) per length of PV_LENGTHS: computed once, never modified."""
    out = []
    for k, L in enumerate(PV_LENGTHS):
        b = gen_bytes(900 + k, L).tobytes()
        out.append((b, hashlib.sha256(b).digest()))
    return out


def _flipped(b, at):
    x = bytearray(b)
    x[at] ^= 0x01
    return bytes(x)


def _mixed_list(copies):
    """Every copy good, flipped in its first byte and flipped in its last byte, in an order that
    puts lengths of every size side by side -> (list entries, digests, expected flags)."""
    entries, digests, want = [], [], []
    for r in range(3):
        for k in range(len(copies)):
            b, dg = copies[(k + 2 * r) % len(copies)]
            entries.append(b if r == 0 else _flipped(b, 0 if r == 1 else len(b) - 1))
            digests.append(dg)
            want.append(1 if r == 0 else 0)
    return entries, digests, bytes(want)


def test_parts_verify_good_and_flipped_copies(copies):
    entries, digests, want = _mixed_list(copies)
    assert ce.parts_verify(entries, digests) == want
    # against the oracle's digests too
    assert all(oracle.sha256(b) == dg for b, dg in copies[:5])
    # one entry alone, of every length
    for b, dg in copies:
        assert ce.parts_verify([b], [dg]) == b"\x01"
        assert ce.parts_verify([_flipped(b, len(b) // 2)], [dg]) == b"\x00"


def test_parts_verify_duplicate_entries_of_one_buffer(copies):
    """A list entry is a copy, not a chunk slot: the same buffer several times, with the right
    and with a wrong digest."""
    b, dg = copies[3]
    big, bdg = copies[5]
    buf = (ctypes.c_uint8 * len(b)).from_buffer_copy(b)
    entries = [buf, big, buf, buf, big]
    digests = [dg, bdg, bytes(32), dg, dg]
    assert ce.parts_verify(entries, digests) == bytes([1, 1, 0, 1, 0])


def test_parts_verify_rounds(knob_env, copies):
    """A 1 MiB cap cuts the list into several rounds, the 2 MiB + 1 copy alone in its own; the
    flags are the same."""
    entries, digests, want = _mixed_list(copies)
    assert sum(len(e) for e in entries) > 6 << 20 and max(len(e) for e in entries) > 1 << 20
    assert ce.parts_verify(entries, digests) == want
    knob_env.set("CEC_COALESCE_MAX_MIB", "1")
    assert ce.parts_verify(entries, digests) == want


def test_parts_verify_four_threads(copies):
    errors = []

    def work(w):
        try:
            entries, digests, want = _mixed_list(copies[:6])
            entries, digests = entries[w:], digests[w:]
            for _ in range(3):
                assert ce.parts_verify(entries, digests) == want[w:]
        except BaseException as e:  # noqa: BLE001  (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,)) for w in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_parts_verify_zero_length_in_the_middle():
    code, untouched = _parts_verify_raw([100, 0, 1000])
    assert code == ce.EMPTY_SHARD and untouched
    # well formed: runs (0xEE copies against zero digests: every flag 0)
    code, untouched = _parts_verify_raw([100, 1, 1000])
    assert code == ce.OK and not untouched
