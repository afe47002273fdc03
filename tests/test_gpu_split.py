"""The split ragged layout on the GPU (cec_encode_hash_split): the data chunks of a batch in one
region, the parity chunks in another, against the CPU oracle.  Integer work: every comparison is
exact.  Both regions are carved from buffers filled with 0xA5, with 64 canary bytes behind each,
and the WHOLE of both is checked afterwards: the parity region holds the oracle's parity over
exactly L_k bytes per chunk and 0xA5 everywhere else, the data region is what went in."""
import numpy as np
import pytest

from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import (CANARY, DEV, LENGTHS, SHAPES, _oracle_parts,  # noqa: E402
                             _stride)

SPLIT_SHAPES = SHAPES + [(3, 10)]  # ten parity rows: two row groups
TAIL = 64


def _first_diff(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0]} "
                             f"(got {got[bad[0]]:#x}, want {want[bad[0]]:#x})")


def _run_split(rs, parts, place="below", doffs=None, poffs=None, db=None, pb=None):
    """One cec_encode_hash_split call over `parts` (_oracle_parts tuples).  place: the parity
    region at a lower address than the data region in one allocation ("below"), at a higher one
    ("above"), or in an allocation of its own ("separate").  Returns (parity region, digests)."""
    d, p = rs.data_shard_count(), rs.parity_shard_count()
    lens = [part[0].shape[1] for part in parts]
    if doffs is None:
        doffs, poffs, db, pb = ce.split_layout(d, p, lens)
    data_in = np.full(db + TAIL, CANARY, np.uint8)
    want_par = np.full(pb + TAIL, CANARY, np.uint8)
    for (data, par, _), do, po, L in zip(parts, doffs, poffs, lens):
        for j in range(d):
            data_in[do + j * _stride(L):do + j * _stride(L) + L] = data[j]
        for i in range(p):
            want_par[po + i * _stride(L):po + i * _stride(L) + L] = par[i]
    if place == "separate":
        dbuf = torch.from_numpy(data_in).to(DEV)
        pbuf = torch.full((pb + TAIL,), CANARY, dtype=torch.uint8, device=DEV)
    else:
        whole = torch.full((db + pb + 2 * TAIL,), CANARY, dtype=torch.uint8, device=DEV)
        first, second = (pb + TAIL, db + TAIL) if place == "below" else (db + TAIL, pb + TAIL)
        lo, hi = whole[:first], whole[first:first + second]
        pbuf, dbuf = (lo, hi) if place == "below" else (hi, lo)
        dbuf.copy_(torch.from_numpy(data_in))
    assert dbuf.data_ptr() % 16 == 0 and pbuf.data_ptr() % 16 == 0
    assert (pbuf.data_ptr() < dbuf.data_ptr()) == (place == "below") or place == "separate"
    dig = torch.zeros((len(parts), d + p, 32), dtype=torch.uint8, device=DEV)
    ce.encode_hash_split(rs, dbuf.data_ptr(), doffs, pbuf.data_ptr(), poffs, lens, dig.data_ptr())
    torch.cuda.synchronize()
    got_par = pbuf.cpu().numpy()
    _first_diff(got_par, want_par, "parity region")
    _first_diff(dbuf.cpu().numpy(), data_in, "data region")
    return got_par, dig.cpu().numpy()


@pytest.fixture(scope="module")
def oracle_batches():
    """One batch per shape, one part per chunk length: computed once, shared, never modified."""
    return {(d, p): _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in SPLIT_SHAPES}


@pytest.mark.parametrize("d,p", SPLIT_SHAPES)
def test_split_matches_oracle_and_writes_nothing_else(d, p, oracle_batches):
    parts = oracle_batches[(d, p)]
    _, dig = _run_split(ce.ReedSolomon(d, p), parts)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), (LENGTHS[k], "digests")


@pytest.mark.parametrize("place", ["above", "separate"])
@pytest.mark.parametrize("d,p", [(3, 2), (10, 4), (3, 10)])
def test_split_parity_region_above_or_apart(d, p, place, oracle_batches):
    parts = oracle_batches[(d, p)]
    _, dig = _run_split(ce.ReedSolomon(d, p), parts, place)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), (LENGTHS[k], "digests")


@pytest.mark.parametrize("place", ["below", "above", "separate"])
def test_split_spaced_offsets(place, oracle_batches):
    """Offsets need not be packed, in either region, and the two need not be spaced alike."""
    d, p = 3, 2
    parts = oracle_batches[(d, p)][:12]
    doffs, poffs, db, pb = ce.split_layout(d, p, LENGTHS[:12])
    doffs = [o + 4096 * k + 16 * (k % 3) for k, o in enumerate(doffs)]
    poffs = [o + 1024 * k + 16 * (k % 5) for k, o in enumerate(poffs)]
    _, dig = _run_split(ce.ReedSolomon(d, p), parts, place, doffs, poffs, db + 4096 * 12 + 64,
                        pb + 1024 * 12 + 80)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig)


@pytest.mark.parametrize("d,p", [(3, 2), (10, 4), (3, 10)])
def test_split_equals_encode_hash_ragged(d, p, oracle_batches):
    parts = oracle_batches[(d, p)]
    rs = ce.ReedSolomon(d, p)
    t = d + p
    got_par, dig = _run_split(rs, parts, "separate")
    doffs, poffs, db, pb = ce.split_layout(d, p, LENGTHS)
    offs, total = ce.ragged_layout(t, LENGTHS)
    host = np.zeros(total, np.uint8)
    for (data, _, _), off, L in zip(parts, offs, LENGTHS):
        for j in range(d):
            host[off + j * _stride(L):off + j * _stride(L) + L] = data[j]
    buf = torch.from_numpy(host).to(DEV)
    rdig = torch.zeros((len(parts), t, 32), dtype=torch.uint8, device=DEV)
    ce.encode_hash_ragged(rs, buf.data_ptr(), offs, LENGTHS, rdig.data_ptr())
    torch.cuda.synchronize()
    ragged = buf.cpu().numpy()
    assert np.array_equal(rdig.cpu().numpy(), dig)
    for off, po, L in zip(offs, poffs, LENGTHS):
        for i in range(p):
            at = off + (d + i) * _stride(L)
            assert np.array_equal(ragged[at:at + L],
                                  got_par[po + i * _stride(L):po + i * _stride(L) + L]), (L, i)


def test_split_one_byte_beside_one_mib():
    d, p = 10, 4
    parts = _oracle_parts(d, p, [1, 1 << 20, 1, 683], 6)
    _, dig = _run_split(ce.ReedSolomon(d, p), parts)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), k


def test_split_4096_one_byte_parts():
    d, p, n = 10, 4, 4096
    parts = _oracle_parts(d, p, [1] * n, 5)
    _, dig = _run_split(ce.ReedSolomon(d, p), parts, "above")
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), k


def test_split_order_independence(oracle_batches):
    """The same parts in a shuffled order give the same results per part (the whole-region check
    of _run_split compares every parity chunk at its shuffled place)."""
    d, p = 10, 4
    parts = oracle_batches[(d, p)]
    order = np.random.default_rng(3).permutation(len(parts))
    _, dig = _run_split(ce.ReedSolomon(d, p), [parts[k] for k in order])
    for q, k in enumerate(order):
        assert np.array_equal(dig[q], parts[k][2]), LENGTHS[k]


def test_split_overlapping_regions_refused_with_nothing_written(oracle_batches):
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    lens = LENGTHS[:8]
    doffs, poffs, db, pb = ce.split_layout(d, p, lens)
    buf = torch.full((db + pb + TAIL,), CANARY, dtype=torch.uint8, device=DEV)
    dig = torch.full((len(lens), d + p, 32), CANARY, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    # the parity region on the data region, into its end, and the data region into the parity's
    for dptr, pptr in ((base, base), (base, base + db - 16), (base + pb - 16, base)):
        with pytest.raises(ce.Error) as e:
            ce.encode_hash_split(rs, dptr, doffs, pptr, poffs, lens, dig.data_ptr())
        assert e.value.code == ce.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and bool((dig == CANARY).all())
    # touching regions are fine (this shape's parity of d equal data chunks is that chunk again,
    # so the data region gets other bytes than the canary first)
    data = torch.from_numpy(gen_bytes(4, db)).to(DEV)
    buf[:db] = data
    ce.encode_hash_split(rs, base, doffs, base + db, poffs, lens, dig.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(buf[:db], data) and bool((buf[db + pb:] == CANARY).all())
    assert not bool((buf[db:db + pb] == CANARY).all())
