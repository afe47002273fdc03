"""tests/_gen.synth_chunk (the numpy mirror of the synthetic-data generator) against the library's
host function cec_synth_byte, point by point: the GPU fill tests compare whole device buffers
with the mirror, so the mirror itself is pinned to the C here, where no GPU is needed."""
import itertools

import numpy as np

import chunky_ec as ce
from _gen import synth_batch, synth_chunk

SEEDS = [0, 1, 2025, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0xDEADBEEFCAFEF00D]
PARTS = [0, 1, 255, 65536, 65537 + 9362, (1 << 32) - 1, (1 << 40) + 3]
CHUNKS = [0, 1, 13, 65535, 65536 + 5, (1 << 32) + 1]
OFFSETS = [0, 7, 8, (1 << 32) - 1, (1 << 32) + 9]


def test_mirror_matches_synth_byte_at_points():
    """Every (seed, part, chunk, offset) of the lists above (1260 points): offsets on both sides
    of a word boundary and of 2^32, part and chunk values above 2^16 and 2^32 (the key's
    multiply wraps), seeds with the top bit set."""
    n = 0
    for seed, part, chunk, off in itertools.product(SEEDS, PARTS, CHUNKS, OFFSETS):
        got = synth_chunk(seed, part, chunk, 1, first=off)
        assert got.dtype == np.uint8 and got.shape == (1,)
        assert int(got[0]) == ce.synth_byte(seed, part, chunk, off), (seed, part, chunk, off)
        n += 1
    assert n == 1260


def test_mirror_whole_chunk_and_window():
    """A whole chunk of an odd length byte by byte (the last word is partial), and a window that
    starts and ends inside words equals the same bytes of the whole chunk."""
    seed, part, chunk, L = 0x9000000000000007, 70001, 66000, 683
    whole = synth_chunk(seed, part, chunk, L)
    assert whole.shape == (L,)
    assert whole.tolist() == [ce.synth_byte(seed, part, chunk, o) for o in range(L)]
    assert np.array_equal(synth_chunk(seed, part, chunk, 100, first=13), whole[13:113])
    assert synth_chunk(seed, part, chunk, 0).shape == (0,)
    # chunks and parts differ from one another (a fill that ignored an index would not)
    assert not np.array_equal(whole, synth_chunk(seed, part, chunk + 1, L))
    assert not np.array_equal(whole, synth_chunk(seed, part + 1, chunk, L))


def test_batch_mirror_equals_chunk_mirror():
    seed = 0xC000000000000001
    for L in (1, 5, 8, 683):
        got = synth_batch(seed, 4, 3, L)
        assert got.shape == (4, 3, L) and got.dtype == np.uint8
        for k in range(4):
            for c in range(3):
                assert np.array_equal(got[k, c], synth_chunk(seed, k, c, L)), (L, k, c)
