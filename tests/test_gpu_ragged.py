"""Ragged batches on the GPU: parts of different chunk lengths encoded and hashed in one launch
sequence (cec_encode_hash_ragged) and the host-staged cec_parts_encode on top of it, against the
CPU oracle and hashlib.  Integer work: every comparison is exact.

The ragged GF(2^8) kernel's work unit is 4096 bytes of one part's columns per wave, walked in
1024-byte steps (64 lanes x one 16-byte column), so the chunk lengths below carry +-1 around
both, beside the 16-byte column edges, SHA-256's padding edges and the 4 / 8 / 16 KiB spans of
the uniform kernels."""
import hashlib
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_ragged import _parts_encode_raw  # noqa: E402

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda", 0)
CANARY = 0xA5
SHAPES = [(1, 1), (3, 2), (10, 4), (5, 5), (17, 3), (20, 8)]
LENGTHS = [1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 683, 1023, 1024, 1025, 4095, 4096, 4097,
           8191, 8192, 8193, 16383, 16384, 16385, 65537]


def _stride(L):
    return (L + 15) // 16 * 16


def _oracle_parts(d, p, lens, seed):
    """(data (d, L), parity (p, L), digests (d+p, 32)) per chunk length, from the CPU oracle."""
    out = []
    for k, L in enumerate(lens):
        data = gen_bytes(seed * 1000 + k, d * L).reshape(d, L)
        cs, par, dig = oracle.part_encode(d, p, data.reshape(-1), d * L)
        assert cs == L
        out.append((data, par, dig))
    return out


def _run_ragged(rs, parts, offs=None, total=None):
    """One cec_encode_hash_ragged call over `parts` (the _oracle_parts tuples) in a device buffer
    filled with 0xA5 before the data goes in.  Checks the WHOLE buffer afterwards: parity chunks
    equal the oracle's over exactly L bytes, and every other byte (the data chunks, the padding
    up to each stride, the space between and behind the parts) is what it was.  Returns the
    digests [n][d+p][32]."""
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    t = d + p
    lens = [part[0].shape[1] for part in parts]
    if offs is None:
        offs, total = ce.ragged_layout(t, lens)
    before = np.full(total + 64, CANARY, np.uint8)  # 64 canary bytes behind the last part
    for (data, par, _), off, L in zip(parts, offs, lens):
        for j in range(d):
            before[off + j * _stride(L):off + j * _stride(L) + L] = data[j]
    want = before.copy()
    for (data, par, _), off, L in zip(parts, offs, lens):
        for i in range(p):
            at = off + (d + i) * _stride(L)
            want[at:at + L] = par[i]
    buf = torch.from_numpy(before).to(DEV)
    dig = torch.zeros((len(parts), t, 32), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    ce.encode_hash_ragged(rs, buf.data_ptr(), offs, lens, dig.data_ptr())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[0]} "
                             f"(got {got[bad[0]]:#x}, want {want[bad[0]]:#x})")
    return dig.cpu().numpy()


@pytest.fixture(scope="module")
def oracle_batches():
    """One batch per shape, one part per chunk length: computed once, shared, never modified."""
    return {(d, p): _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in SHAPES}


@pytest.mark.parametrize("d,p", SHAPES)
def test_ragged_matches_oracle_and_keeps_canary(d, p, oracle_batches):
    parts = oracle_batches[(d, p)]
    dig = _run_ragged(ce.ReedSolomon(d, p), parts)
    for k, (data, par, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), (LENGTHS[k], "digests")
        assert dig[k, 0].tobytes() == hashlib.sha256(data[0].tobytes()).digest()


def test_ragged_spaced_offsets(oracle_batches):
    """Offsets need not be packed: parts with unused space between them."""
    d, p = 3, 2
    parts = oracle_batches[(d, p)][:12]
    lens = LENGTHS[:12]
    offs, total = ce.ragged_layout(d + p, lens)
    offs = [o + 4096 * k + 16 * (k % 3) for k, o in enumerate(offs)]
    dig = _run_ragged(ce.ReedSolomon(d, p), parts, offs, total + 4096 * 12 + 64)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig)


def test_ragged_uniform_equals_encode_hash_batch():
    d, p, n, L = 10, 4, 8, 4096
    t = d + p
    rs = ce.ReedSolomon(d, p)
    data = gen_bytes(77, n * d * L).reshape(n, d, L)
    a = torch.zeros((n, t, L), dtype=torch.uint8, device=DEV)
    a[:, :d] = torch.from_numpy(data).to(DEV)
    b = a.clone()
    dig_a = torch.zeros((n, t, 32), dtype=torch.uint8, device=DEV)
    dig_b = torch.zeros_like(dig_a)
    ce.encode_hash_batch(rs, ce.PartBatch.from_tensor(a, L), dig_a.data_ptr())
    offs, total = ce.ragged_layout(t, [L] * n)
    assert offs == [k * t * L for k in range(n)] and total == n * t * L
    ce.encode_hash_ragged(rs, b.data_ptr(), offs, [L] * n, dig_b.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(dig_a, dig_b)
    assert bool((b[:, d:] != 0).any())


def test_ragged_4096_one_byte_parts():
    d, p, n = 10, 4, 4096
    parts = _oracle_parts(d, p, [1] * n, 5)
    dig = _run_ragged(ce.ReedSolomon(d, p), parts)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), k


def test_ragged_one_byte_beside_one_mib():
    d, p = 10, 4
    parts = _oracle_parts(d, p, [1, 1 << 20, 1, 683], 6)
    dig = _run_ragged(ce.ReedSolomon(d, p), parts)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), k


def test_ragged_order_independence(oracle_batches):
    """The same parts in a shuffled order give the same results per part (a length sort that
    misplaced digests would not)."""
    d, p = 10, 4
    parts = oracle_batches[(d, p)]
    order = np.random.default_rng(3).permutation(len(parts))
    assert list(order) != sorted(order)
    rs = ce.ReedSolomon(d, p)
    dig = _run_ragged(rs, parts)
    dig_s = _run_ragged(rs, [parts[i] for i in order])
    for pos, i in enumerate(order):
        assert np.array_equal(dig_s[pos], dig[i])
        assert np.array_equal(dig_s[pos], parts[i][2])


# ----------------------------------------------------------------------------------------------
# cec_parts_encode (host staged)
# ----------------------------------------------------------------------------------------------

def _check_parts(d, p, bufs, encs):
    assert len(encs) == len(bufs)
    for buf, enc in zip(bufs, encs):
        cs, par, dig = oracle.part_encode(d, p, np.frombuffer(buf, np.uint8), len(buf))
        assert enc.chunksize == cs == (len(buf) + d - 1) // d
        assert [bytes(x) for x in enc.parity] == [par[i].tobytes() for i in range(p)], len(buf)
        assert [h.digest for h in enc.hashes] == [dig[i].tobytes() for i in range(d + p)], len(buf)
        # the last data chunk as the engine must have padded it: the caller's bytes, then zeros
        last = buf[(d - 1) * cs:].ljust(cs, b"\0")
        assert enc.hashes[d - 1].digest == hashlib.sha256(last).digest()


@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_parts_encode_equals_part_encode(d, p):
    rs = ce.ReedSolomon(d, p)
    L = 4096
    lengths = [1, 2, 7, 20480, 699051 * 3, d * L, d * L - (d - 1)]
    # exactly `length` bytes each: the zero padding up to d * chunksize is the engine's
    bufs = [gen_bytes(40 + k, n).tobytes() for k, n in enumerate(lengths)]
    encs = ce.parts_encode(rs, bufs)
    _check_parts(d, p, bufs, encs)
    for buf, enc in zip(bufs[:4] + bufs[5:], encs[:4] + encs[5:]):
        one = ce.part_encode(rs, buf, len(buf))
        assert one.chunksize == enc.chunksize and one.parity == enc.parity
        assert [h.digest for h in one.hashes] == [h.digest for h in enc.hashes]


def test_parts_encode_parity_copy_back_merge_boundary():
    """The parity comes back from the device in copies that neighbouring parts share until the
    data chunks between two parts' parity reach 256 KiB.  RS(3,2) chunk lengths that put that gap
    (d * stride) just under it (262 128), just over it (262 176) and on an unaligned length with
    the same stride, 16-byte parts between them: every part's parity must still arrive."""
    d, p = 3, 2
    chunk_lens = [16, 87376, 16, 87392, 16, 87381, 16]
    assert [d * _stride(L) for L in chunk_lens[1::2]] == [262128, 262176, 262176]
    assert 262128 < (256 << 10) < 262176
    bufs = [gen_bytes(80 + k, d * L).tobytes() for k, L in enumerate(chunk_lens)]
    encs = ce.parts_encode(ce.ReedSolomon(d, p), bufs)
    _check_parts(d, p, bufs, encs)


def test_parts_encode_rounds(knob_env):
    """A 1 MiB cap cuts about 3 MiB of parts plus one 2 MiB part into several rounds (the large
    part alone); the results are the same."""
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    sizes = [200_001, 350_017, 1, 2 << 20, 420_000, 683, 510_003, 99_999, 640_000, 333_333,
             250_000, 300_000]
    assert 3_000_000 < sum(sizes) - (2 << 20) < 3_500_000
    bufs = [gen_bytes(60 + k, n).tobytes() for k, n in enumerate(sizes)]
    want = ce.parts_encode(rs, bufs)
    knob_env.set("CEC_COALESCE_MAX_MIB", "1")
    got = ce.parts_encode(rs, bufs)
    _check_parts(d, p, bufs, got)
    assert [(e.chunksize, e.parity, [h.digest for h in e.hashes]) for e in got] == \
        [(e.chunksize, e.parity, [h.digest for h in e.hashes]) for e in want]


def test_parts_encode_four_threads():
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    jobs = [[gen_bytes(100 * w + k, n).tobytes()
             for k, n in enumerate([1 + w, 4097 * (w + 1), 70_001, 683, 20480 + w])]
            for w in range(4)]
    results, errors = [None] * 4, []

    def work(w):
        try:
            results[w] = ce.parts_encode(rs, jobs[w])
        except Exception as e:  # noqa: BLE001  (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,)) for w in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for w in range(4):
        _check_parts(d, p, jobs[w], results[w])


def test_parts_encode_zero_length_in_the_middle():
    rs = ce.ReedSolomon(3, 2)
    code, untouched = _parts_encode_raw(rs, [b"abc" * 100, b"", b"xyz" * 1000])
    assert code == ce.EMPTY_SHARD and untouched
    code, untouched = _parts_encode_raw(rs, [b"abc" * 100, b"q", b"xyz" * 1000])
    assert code == ce.OK and not untouched
