"""Deterministic test inputs (splitmix64 over numpy uint64; independent of numpy's RNG streams).

Used by tests/golden/make_golden.py and the parity tests, so committed fixtures can always be
regenerated bit for bit.
"""
import numpy as np

_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_G = np.uint64(0x9E3779B97F4A7C15)


def _mix(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * _M1
        z = z ^ (z >> np.uint64(27))
        z = z * _M2
        z = z ^ (z >> np.uint64(31))
    return z


def gen_bytes(seed: int, n: int) -> np.ndarray:
    """n pseudo-random bytes for `seed` (little-endian bytes of splitmix64(seed*G + i))."""
    words = (n + 7) // 8
    with np.errstate(over="ignore"):
        idx = np.arange(words, dtype=np.uint64) + np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * _G
    return _mix(idx).view(np.uint8)[:n].copy()


_SYNTH_PART = np.uint64(0x100000001B3)
_U64 = 0xFFFFFFFFFFFFFFFF


def _synth_words(seed: int, part: np.ndarray, chunk: np.ndarray, word: np.ndarray) -> np.ndarray:
    """mix64 / synth_key / synth_word of csrc/rs_kernels.hip over uint64 arrays (broadcast), which
    wrap as the C does: synth_word(synth_key(seed, part, chunk), word)."""
    with np.errstate(over="ignore"):
        key = _mix(np.uint64(seed & _U64) ^ _mix(part * _SYNTH_PART + chunk + _G))
        return _mix(key + word * _G)


def synth_chunk(seed: int, part: int, chunk: int, length: int, first: int = 0) -> np.ndarray:
    """uint8[length]: bytes [first, first + length) of chunk `chunk` of part `part` as
    cec_fill_synthetic(seed) writes them (byte o is byte o % 8, little-endian, of word o / 8)."""
    w0, w1 = first // 8, (first + length + 7) // 8
    words = _synth_words(seed, np.array([part & _U64], np.uint64),
                         np.array([chunk & _U64], np.uint64), np.arange(w0, w1, dtype=np.uint64))
    lo = first - w0 * 8
    return words.astype("<u8").view(np.uint8)[lo:lo + length].copy()


def synth_batch(seed: int, n_parts: int, n_chunks: int, length: int) -> np.ndarray:
    """uint8[n_parts][n_chunks][length]: synth_chunk of every (part, chunk), in one pass."""
    words = (length + 7) // 8
    w = _synth_words(seed, np.arange(n_parts, dtype=np.uint64)[:, None, None],
                     np.arange(n_chunks, dtype=np.uint64)[None, :, None],
                     np.arange(words, dtype=np.uint64)[None, None, :])
    out = np.ascontiguousarray(w.astype("<u8")).view(np.uint8)
    return out.reshape(n_parts, n_chunks, words * 8)[:, :, :length].copy()


def cluster_reader_bytes() -> bytes:
    """tests/cluster.rs:95-102 `default_reader`: 80 blocks of 256 bytes, byte = (x % 128) + i."""
    out = bytearray()
    for i in range(80):
        out += bytes(((x % 128) + i) & 0xFF for x in range(256))
    return bytes(out)
