"""The ragged write pipeline on the GPU (cec_parts_pipeline_*): batches of parts of different
chunk lengths through slots in flight, against the CPU oracle and cec_parts_encode on the same
bytes.  Integer work: every comparison is exact."""
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import LENGTHS, _stride  # noqa: E402

SHAPES = [(3, 2), (10, 4)]
SLOT, MAX_PARTS, DEPTH, BATCHES = 1 << 20, 64, 2, 7


def _files(d, seed):
    """Per batch, one file per chunk length of LENGTHS[b::BATCHES]: d * L - r bytes with r < d, so
    its chunk size is L and most files end inside their last chunk."""
    out = []
    for b in range(BATCHES):
        bufs = []
        for q, L in enumerate(LENGTHS[b::BATCHES]):
            n = d * L - (q + b) % d
            bufs.append(gen_bytes(seed * 100 + b * 10 + q, n).tobytes())
        out.append(bufs)
    return out


@pytest.fixture(scope="module")
def reference():
    """Per shape: the batches' files and, per file, the oracle's (chunksize, parity, digests):
    computed once, shared, never modified."""
    ref = {}
    for d, p in SHAPES:
        files = _files(d, 10 * d + p)
        ref[(d, p)] = (files, [[oracle.part_encode(d, p, np.frombuffer(f, np.uint8), len(f))
                                for f in bufs] for bufs in files])
    return ref


def _results(pl, slot, chunk_lens):
    """wait(slot) unpacked: per part (p parity chunks as bytes, digests (d+p, 32) copy)."""
    parity, digests = pl.wait(slot)
    assert digests.shape == (len(chunk_lens), pl.d + pl.p, 32)
    _, poffs, _, pb = ce.split_layout(pl.d, pl.p, chunk_lens) if chunk_lens else ([], [], 0, 0)
    assert parity.shape == (pb,)
    out = []
    for k, L in enumerate(chunk_lens):
        cs = _stride(L)
        out.append(([parity[poffs[k] + i * cs:poffs[k] + i * cs + L].tobytes()
                     for i in range(pl.p)], digests[k].copy()))
    return out


def _check(got, want, chunk_lens):
    assert len(got) == len(want)
    for (par, dig), (cs, opar, odig), L in zip(got, want, chunk_lens):
        assert cs == L
        assert [bytes(x) for x in opar] == par, (L, "parity")
        assert np.array_equal(dig, odig), (L, "digests")


def _fill(pl, data, bufs):
    """The caller's packing for submit: the packed split layout, zeros behind a file's bytes."""
    d = pl.d
    lens = [(len(b) + d - 1) // d for b in bufs]
    doffs, _, db, _ = ce.split_layout(d, pl.p, lens)
    data[:db] = 0xA5  # what lies between chunks is never read
    for b, off, L in zip(bufs, doffs, lens):
        padded = np.zeros(d * L, np.uint8)
        padded[:len(b)] = np.frombuffer(b, np.uint8)
        for j in range(d):
            data[off + j * _stride(L):off + j * _stride(L) + L] = padded[j * L:(j + 1) * L]
    return lens


def _stream(pl, files, want, use_submit=False):
    """Every batch through the pipeline with all slots in flight, the oldest collected first."""
    pending, results, first = [], [], None

    def collect():
        slot, lens, b = pending.pop(0)
        got = _results(pl, slot, lens)
        _check(got, want[b], lens)
        results.append(got)
    for b, bufs in enumerate(files):
        if len(pending) == pl.depth:
            collect()
        slot, data = pl.acquire()
        first = slot if first is None else first
        assert slot == (first + b) % pl.depth  # round-robin from wherever the pipeline stood
        assert data.shape == (pl.slot_data_bytes,)
        if use_submit:
            lens = _fill(pl, data, bufs)
            pl.submit(slot, lens)
        else:
            lens = pl.submit_from(slot, bufs)
        pending.append((slot, lens, b))
    while pending:
        collect()
    return results


@pytest.mark.parametrize("d,p", SHAPES)
def test_seven_batches_equal_oracle_and_parts_encode(d, p, reference):
    files, want = reference[(d, p)]
    rs = ce.ReedSolomon(d, p)
    pl = ce.PartsPipeline(rs, SLOT, MAX_PARTS, DEPTH)
    assert pl.depth == DEPTH == ce._lib.cec_parts_pipeline_depth(pl._h)
    results = _stream(pl, files, want)  # 7 batches on 2 slots: each slot at least three times
    for bufs, got in zip(files, results):
        enc = ce.parts_encode(rs, bufs)
        for e, (par, dig) in zip(enc, got):
            assert e.parity == par
            assert [h.digest for h in e.hashes] == [dig[i].tobytes() for i in range(d + p)]


@pytest.mark.parametrize("d,p", SHAPES)
def test_submit_equals_submit_from(d, p, reference):
    files, want = reference[(d, p)]
    pl = ce.PartsPipeline(ce.ReedSolomon(d, p), SLOT, MAX_PARTS, DEPTH)
    a = _stream(pl, files, want, use_submit=True)
    b = _stream(pl, files, want)
    for ga, gb in zip(a, b):
        for (pa, da), (pb, db) in zip(ga, gb):
            assert pa == pb and np.array_equal(da, db)


@pytest.mark.parametrize("d,p", SHAPES)
def test_results_stay_until_the_slot_is_acquired_again(d, p, reference):
    files, want = reference[(d, p)]
    pl = ce.PartsPipeline(ce.ReedSolomon(d, p), SLOT, MAX_PARTS, DEPTH)
    s0, _ = pl.acquire()
    lens0 = pl.submit_from(s0, files[0])
    parity0, digests0 = pl.wait(s0)
    keep_par, keep_dig = parity0.copy(), digests0.copy()
    s1, _ = pl.acquire()
    assert (s0, s1) == (0, 1)
    lens1 = pl.submit_from(s1, files[3])
    _check(_results(pl, s1, lens1), want[3], lens1)
    # slot 0's views are still its batch, while and after slot 1 ran
    assert np.array_equal(parity0, keep_par) and np.array_equal(digests0, keep_dig)
    _check(_results(pl, s0, lens0), want[0], lens0)
    s2, _ = pl.acquire()
    assert s2 == 0
    lens2 = pl.submit_from(s2, files[1])
    _check(_results(pl, s2, lens2), want[1], lens2)
    assert not np.array_equal(digests0[:1], keep_dig[:1])  # gone: the new batch's


@pytest.mark.parametrize("d,p", SHAPES)
def test_slot_capacity_and_refused_batches(d, p, reference):
    files, want = reference[(d, p)]
    rs = ce.ReedSolomon(d, p)
    pl = ce.PartsPipeline(rs, SLOT, MAX_PARTS, DEPTH)
    # the largest single part the slot takes, and one 16-byte column more
    S = SLOT // (d * 16) * 16
    big = gen_bytes(99, d * S).tobytes()
    slot, _ = pl.acquire()
    assert pl.submit_from(slot, [big]) == [S]
    cs, opar, odig = oracle.part_encode(d, p, np.frombuffer(big, np.uint8), len(big))
    _check(_results(pl, slot, [S]), [(cs, opar, odig)], [S])
    slot, _ = pl.acquire()
    for call in (lambda: pl.submit_from(slot, [big + b"x"]), lambda: pl.submit(slot, [S + 1]),
                 lambda: pl.submit(slot, [S, 1])):
        with pytest.raises(ce.Error) as e:
            call()
        assert e.value.code == ce.ERR_INVALID_ARGUMENT
    # too many parts, a zero length in the middle: refused, and the slot then takes a batch
    for call, code in ((lambda: pl.submit_from(slot, [b"a"] * (MAX_PARTS + 1)),
                        ce.ERR_INVALID_ARGUMENT),
                       (lambda: pl.submit(slot, [1] * (MAX_PARTS + 1)), ce.ERR_INVALID_ARGUMENT),
                       (lambda: pl.submit_from(slot, [b"a", b"", b"c"]), ce.EMPTY_SHARD),
                       (lambda: pl.submit(slot, [16, 0, 16]), ce.EMPTY_SHARD)):
        with pytest.raises(ce.Error) as e:
            call()
        assert e.value.code == code
    lens = pl.submit_from(slot, files[2])
    _check(_results(pl, slot, lens), want[2], lens)
    full = [b"a"] * MAX_PARTS  # max_parts itself is fine
    slot, _ = pl.acquire()
    assert pl.submit_from(slot, full) == [1] * MAX_PARTS
    assert pl.wait(slot)[1].shape == (MAX_PARTS, d + p, 32)
    # a slot that a batch fills exactly, and one that the same batch exceeds by 16 bytes
    L = 4097
    part = gen_bytes(98, d * L).tobytes()
    ref = [oracle.part_encode(d, p, np.frombuffer(part, np.uint8), len(part))]
    exact = ce.PartsPipeline(rs, d * _stride(L), 1, 1)
    slot, _ = exact.acquire()
    assert exact.submit_from(slot, [part]) == [L]
    _check(_results(exact, slot, [L]), ref, [L])
    short = ce.PartsPipeline(rs, d * _stride(L) - 16, 1, 1)
    slot, _ = short.acquire()
    with pytest.raises(ce.Error) as e:
        short.submit_from(slot, [part])
    assert e.value.code == ce.ERR_INVALID_ARGUMENT
    small = part[:d * 4080]
    assert short.submit_from(slot, [small]) == [4080]
    _check(_results(short, slot, [4080]),
           [oracle.part_encode(d, p, np.frombuffer(small, np.uint8), len(small))], [4080])


def test_empty_batch_query_and_drain(reference):
    d, p = 3, 2
    files, want = reference[(d, p)]
    pl = ce.PartsPipeline(ce.ReedSolomon(d, p), SLOT, MAX_PARTS, DEPTH)
    assert pl.query(0) and pl.query(1)  # nothing in flight
    parity, digests = pl.wait(0)  # a slot with no batch: no parts, at once
    assert parity.shape == (0,) and digests.shape == (0, d + p, 32)
    pl.drain()
    slot, _ = pl.acquire()
    assert pl.submit_from(slot, []) == []
    pl.submit(slot, [])
    assert pl.query(slot)
    assert pl.wait(slot)[1].shape == (0, d + p, 32)
    slot, _ = pl.acquire()
    lens = pl.submit_from(slot, files[4])
    assert pl.query(slot) in (True, False)  # never blocks, whatever the batch's state
    other, _ = pl.acquire()
    lens_o = pl.submit_from(other, files[5])
    pl.drain()
    assert pl.query(slot) and pl.query(other)
    _check(_results(pl, slot, lens), want[4], lens)
    _check(_results(pl, other, lens_o), want[5], lens_o)
    assert pl.query(slot)
    for call in (lambda: pl.query(DEPTH), lambda: pl.wait(DEPTH), lambda: pl.submit(DEPTH, [16])):
        with pytest.raises(ce.Error) as e:
            call()
        assert e.value.code == ce.ERR_INVALID_ARGUMENT


def test_two_threads_each_with_a_pipeline_on_one_codec(reference):
    d, p = 10, 4
    files, want = reference[(d, p)]
    rs = ce.ReedSolomon(d, p)
    pipes = [ce.PartsPipeline(rs, SLOT, MAX_PARTS, DEPTH) for _ in range(2)]  # made up front
    errors = []

    def run(pl, order):
        try:
            _stream(pl, [files[b] for b in order], [want[b] for b in order])
        except BaseException as exc:  # noqa: BLE001  (reported by the main thread)
            errors.append(exc)
    threads = [threading.Thread(target=run, args=(pipes[0], list(range(BATCHES)))),
               threading.Thread(target=run, args=(pipes[1], list(range(BATCHES))[::-1]))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
