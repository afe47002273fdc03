"""The fused ragged encode + SHA-256 kernel on the GPU (encode_hash_ragged_kernel), reached through
cec_encode_hash_ragged, cec_encode_hash_split, cec_parts_encode and cec_parts_pipeline_* under
CEC_RAGGED_FUSED, against the CPU oracle, hashlib and the two-pass path.  Integer work: every
comparison is exact.

The buffers are the whole-buffer pattern of test_gpu_ragged.py / test_gpu_split.py: filled with
0xA5, 64 canary bytes behind them, and compared entirely afterwards, so a byte written into the
padding up to a stride, between two parts or behind the last one fails the test.

The kernel walks a group of G parts in steps of 256 bytes (128 where the LDS ring of a wide shape
needs it), 16-byte columns with a byte path for a chunk's last 1-15 bytes, and every SHA lane pads
its own chunk at its own last step; the chunk lengths below carry the column edges, SHA-256's
padding edges (55 / 56 / 63 / 64 and the same behind one block), both step sizes +-1 and their
doubles, and one chunk of 257 steps in a group of chunks of one."""
import hashlib
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import (_check_parts, _oracle_parts, _run_ragged,  # noqa: E402
                             _stride)
from test_gpu_split import _run_split  # noqa: E402

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

KNOB = "CEC_RAGGED_FUSED"
SHAPES = [(1, 1), (3, 2), (10, 4), (5, 5), (16, 8), (8, 8)]  # (8, 8): 128-byte steps
LENGTHS = [1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 255, 256, 257, 511, 512,
           513, 683, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385,
           65537]


def _group(d, p):
    """Parts per workgroup and step size as the launch picks them: 256-byte steps when the ring
    [2][G * t][STEP + 16] and the 16 product tables fit 160 KiB of LDS, else 128."""
    t = d + p
    for step in (256, 128):
        g = min(256 // t, 256 // (step // 16))
        if 2 * g * t * (step + 16) + 16 * 256 * (4 if p <= 4 else 8) <= 160 * 1024:
            return g, step
    raise AssertionError((d, p))


def _moved(before):
    f, s = ce.ragged_stats()
    return f - before[0], s - before[1]


def _digests_match(dig, parts):
    for k, (data, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), (k, data.shape[1], "digests")
        assert dig[k, 0].tobytes() == hashlib.sha256(data[0].tobytes()).digest()


@pytest.fixture(scope="module")
def oracle_batches():
    """One batch per shape, one part per chunk length: computed once, shared, never modified."""
    return {(d, p): _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in SHAPES}


def test_stats_follow_the_knob(knob_env):
    """One launch sequence per call, counted by the path it took."""
    assert _group(10, 4) == (16, 256) and _group(16, 8) == (10, 256) and _group(8, 8) == (16, 128)
    lens = [257, 1, 4097]
    parts = _oracle_parts(3, 2, lens, 9)
    rs = ce.ReedSolomon(3, 2)
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    _digests_match(_run_ragged(rs, parts), parts)
    assert _moved(before) == (1, 0)
    _digests_match(_run_split(rs, parts)[1], parts)
    assert _moved(before) == (2, 0)
    knob_env.set(KNOB, "0")
    before = ce.ragged_stats()
    _digests_match(_run_ragged(rs, parts), parts)
    _digests_match(_run_split(rs, parts)[1], parts)
    assert _moved(before) == (0, 2)
    # forced on shapes the kernel does not cover: two passes, right results
    knob_env.set(KNOB, "1")
    for d, p in [(17, 3), (20, 8), (3, 10)]:
        wide = _oracle_parts(d, p, lens, 10 * d + p)
        before = ce.ragged_stats()
        _digests_match(_run_ragged(ce.ReedSolomon(d, p), wide), wide)
        assert _moved(before) == (0, 1), (d, p)
    # any other value counts as unset, and unset a launch of 8 parts is a small one: two passes
    eight = _oracle_parts(3, 2, [257] * 8, 11)
    for value in ("2", "10", "", None):
        if value is None:
            knob_env.delenv(KNOB)
        else:
            knob_env.set(KNOB, value)
        before = ce.ragged_stats()
        _digests_match(_run_ragged(rs, eight), eight)
        assert _moved(before) == (0, 1), value


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("d,p", SHAPES)
def test_fused_matches_oracle_and_two_pass(d, p, shuffled, oracle_batches, knob_env):
    parts = oracle_batches[(d, p)]
    if shuffled:
        order = np.random.default_rng(100 * d + p).permutation(len(parts))
        assert list(order) != sorted(order)
        parts = [parts[i] for i in order]
    rs = ce.ReedSolomon(d, p)
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    dig = _run_ragged(rs, parts)  # the whole buffer against the oracle's bytes
    assert _moved(before) == (1, 0)
    _digests_match(dig, parts)
    knob_env.set(KNOB, "0")
    dig0 = _run_ragged(rs, parts)  # the same expected buffer: identical bytes
    assert _moved(before) == (1, 1)
    assert np.array_equal(dig, dig0)


@pytest.fixture(scope="module")
def parts_257():
    g, _ = _group(10, 4)
    return _oracle_parts(10, 4, [257] * (2 * g + 1), 21)


@pytest.mark.parametrize("which", ["one", "G-1", "G", "G+1", "2G+1"])
def test_group_edges(which, parts_257, knob_env):
    g, step = _group(10, 4)
    assert (g, step) == (16, 256)
    n = {"one": 1, "G-1": g - 1, "G": g, "G+1": g + 1, "2G+1": 2 * g + 1}[which]
    parts = parts_257[:n]
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    _digests_match(_run_ragged(ce.ReedSolomon(10, 4), parts), parts)
    assert _moved(before) == (1, 0)


def test_4096_one_byte_parts(knob_env):
    d, p, n = 10, 4, 4096
    parts = _oracle_parts(d, p, [1] * n, 5)
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    dig = _run_ragged(ce.ReedSolomon(d, p), parts)
    assert _moved(before) == (1, 0)
    for k, (_, _, odig) in enumerate(parts):
        assert np.array_equal(dig[k], odig), k


@pytest.mark.parametrize("place", ["below", "above"])
@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_split_layout(d, p, place, oracle_batches, knob_env):
    """_run_split compares the whole parity region (canary included) with the oracle's parity
    over exactly L bytes per chunk, and the whole data region with what went in."""
    parts = oracle_batches[(d, p)]
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    par, dig = _run_split(ce.ReedSolomon(d, p), parts, place)
    assert _moved(before) == (1, 0)
    _digests_match(dig, parts)
    knob_env.set(KNOB, "0")
    par0, dig0 = _run_split(ce.ReedSolomon(d, p), parts, place)
    assert np.array_equal(par, par0) and np.array_equal(dig, dig0)


def test_spaced_offsets(oracle_batches, knob_env):
    """Offsets need not be packed: parts with unused space between them, none of it written."""
    d, p = 3, 2
    parts = oracle_batches[(d, p)][:12]
    lens = LENGTHS[:12]
    offs, total = ce.ragged_layout(d + p, lens)
    offs = [o + 4096 * k + 16 * (k % 3) for k, o in enumerate(offs)]
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    dig = _run_ragged(ce.ReedSolomon(d, p), parts, offs, total + 4096 * 12 + 64)
    assert _moved(before) == (1, 0)
    _digests_match(dig, parts)


# ----------------------------------------------------------------------------------------------
# host staged: cec_parts_encode and the parts pipeline on the fused path
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,p", [(3, 2), (10, 4)])
def test_parts_encode_equals_part_encode(d, p, knob_env):
    rs = ce.ReedSolomon(d, p)
    lengths = [1, 2, 7, 20480, 699051 * 3, d * 4096, d * 4096 - (d - 1)]
    bufs = [gen_bytes(40 + k, n).tobytes() for k, n in enumerate(lengths)]
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    encs = ce.parts_encode(rs, bufs)
    assert _moved(before) == (1, 0)
    _check_parts(d, p, bufs, encs)
    for buf, enc in zip(bufs, encs):
        one = ce.part_encode(rs, buf, len(buf))
        assert one.chunksize == enc.chunksize and one.parity == enc.parity
        assert [h.digest for h in one.hashes] == [h.digest for h in enc.hashes]


def test_parts_encode_four_threads(knob_env):
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    jobs = [[gen_bytes(100 * w + k, n).tobytes()
             for k, n in enumerate([1 + w, 4097 * (w + 1), 70_001, 683, 20480 + w])]
            for w in range(4)]
    results, errors = [None] * 4, []
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()

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
    assert _moved(before) == (4, 0)
    for w in range(4):
        _check_parts(d, p, jobs[w], results[w])


def _pipeline_run(rs, batches):
    """Three submits on two slots, both in flight, the oldest collected first: per batch the
    slot's parity region, the digests and the chunk lengths."""
    pl = ce.PartsPipeline(rs, 1 << 20, 64, 2)
    pending, out = [], []

    def collect():
        slot, lens = pending.pop(0)
        parity, digests = pl.wait(slot)
        out.append((parity.copy(), digests.copy(), lens))
    for bufs in batches:
        if len(pending) == pl.depth:
            collect()
        slot, _ = pl.acquire()
        pending.append((slot, pl.submit_from(slot, bufs)))
    while pending:
        collect()
    return out


def test_parts_pipeline_equals_two_pass(knob_env):
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    batches = [[gen_bytes(500 + 50 * b + q, d * L - (q + b) % d).tobytes()
                for q, L in enumerate(LENGTHS[b:-1:3])] for b in range(3)]
    knob_env.set(KNOB, "1")
    before = ce.ragged_stats()
    got = _pipeline_run(rs, batches)
    assert _moved(before) == (3, 0)
    knob_env.set(KNOB, "0")
    want = _pipeline_run(rs, batches)
    assert _moved(before) == (3, 3)
    for bufs, (par, dig, lens), (par0, dig0, lens0) in zip(batches, got, want):
        assert lens == lens0 == [(len(b) + d - 1) // d for b in bufs]
        assert np.array_equal(dig, dig0)
        # (the padding between the chunks of a slot's pinned parity region is never written)
        _, poffs, _, pb = ce.split_layout(d, p, lens)
        assert par.shape == par0.shape == (pb,)
        for k, buf in enumerate(bufs):
            cs, opar, odig = oracle.part_encode(d, p, np.frombuffer(buf, np.uint8), len(buf))
            assert np.array_equal(dig[k], odig), (lens[k], "digests")
            for i in range(p):
                at = poffs[k] + i * _stride(cs)
                assert par[at:at + cs].tobytes() == par0[at:at + cs].tobytes() == \
                    opar[i].tobytes(), (lens[k], i)
