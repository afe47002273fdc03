"""cec_part_read on the GPU: cec_parts_read for one part, coalesced.  Against the CPU oracle's
chunks and against cec_parts_read(n_parts = 1) on the same inputs slot for slot (the slots
neither call may write included), alone and with 48 concurrent callers of mixed chunk lengths and
mixed damage.  Integer work: every comparison is exact."""
import ctypes
import itertools
import threading

import numpy as np
import pytest

import oracle
from _gen import gen_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

FILL = 0xEE
VERIFIED = ce.PRESENT_VERIFIED
_PARTS = {}


def _part(d, p, L):
    """(chunks (d+p, L), digests bytes) as the oracle stores the part: computed once, shared,
    never modified."""
    key = (d, p, L)
    if key not in _PARTS:
        data = gen_bytes(300 + 7 * L + d, d * L)
        cs, par, dig = oracle.part_encode(d, p, data, d * L)
        assert cs == L
        _PARTS[key] = (np.concatenate([data.reshape(d, L), np.stack(par)]),
                       b"".join(x.tobytes() for x in dig))
    return _PARTS[key]


class Call:
    """One part's arguments: every slot caller memory, a loaded chunk copied in (its last byte
    flipped if listed in `flip`), 0xEE elsewhere."""

    def __init__(self, d, p, L, flags, data_only, flip=()):
        self.d, self.t, self.L, self.data_only = d, d + p, L, data_only
        self.chunks, self.expected = _part(d, p, L)
        self.flags = bytes(flags)
        self.flip = set(flip)
        self.slots = []
        for i in range(self.t):
            s = (ctypes.c_uint8 * L)()
            if flags[i]:
                c = self.chunks[i].copy()
                if i in self.flip:
                    c[-1] ^= 0x80
                ctypes.memmove(s, c.tobytes(), L)
            else:
                ctypes.memset(s, FILL, L)
            self.slots.append(s)
        self.held = [bytes(s) for s in self.slots]
        self.ptrs = (ce._u8p * self.t)(*[ctypes.cast(s, ce._u8p) for s in self.slots])
        self.verified = (ctypes.c_uint8 * self.t)(*([FILL] * self.t))
        self.code = None

    def _args(self):
        return (ctypes.cast(ctypes.c_char_p(self.flags), ce._u8p),
                ctypes.cast(ctypes.c_char_p(self.expected), ce._u8p), 1 if self.data_only else 0)

    def part_read(self, rs):
        self.code = ce._lib.cec_part_read(rs.handle, self.ptrs, self.L, *self._args(),
                                          self.verified)
        return self

    def parts_read(self, rs):
        status = (ctypes.c_int * 1)(77)
        code = ce._lib.cec_parts_read(rs.handle, self.ptrs, (ctypes.c_size_t * 1)(self.L), 1,
                                      *self._args(), self.verified, status)
        assert code == ce.OK
        self.code = status[0]
        return self

    def result(self):
        return self.code, bytes(self.verified), [bytes(s) for s in self.slots]

    def check_against_oracle(self):
        """Verified = loaded and not damaged (a trusted chunk is never hashed); with d verified
        the slots the mode fills equal the oracle's chunks; every other slot keeps its bytes."""
        ver = [1 if self.flags[i] and (i not in self.flip or self.flags[i] == VERIFIED) else 0
               for i in range(self.t)]
        assert list(self.verified) == ver
        ok = sum(ver) >= self.d
        assert self.code == (ce.OK if ok else ce.TOO_FEW_SHARDS_PRESENT)
        for i in range(self.t):
            if ok and not ver[i] and (i < self.d or not self.data_only):
                assert bytes(self.slots[i]) == self.chunks[i].tobytes(), (i, "rebuilt")
            else:
                assert bytes(self.slots[i]) == self.held[i], (i, "untouched")


@pytest.mark.parametrize("data_only", [True, False], ids=["read", "resilver"])
@pytest.mark.parametrize("L", [1, 17, 4099])
def test_every_erasure_pattern_of_rs32(L, data_only):
    d, p = 3, 2
    rs = ce.ReedSolomon(d, p)
    for flags in itertools.product([0, 1], repeat=d + p):
        one = Call(d, p, L, flags, data_only).part_read(rs)
        one.check_against_oracle()
        many = Call(d, p, L, flags, data_only).parts_read(rs)
        assert one.result() == many.result(), flags
    # a loaded chunk that fails verification in a decodable part: rebuilt into its own slot
    for flags, flip in (((1, 1, 1, 1, 0), (1,)), ((1, 1, 1, 1, 1), (0, 4)), ((0, 1, 1, 1, 1), (3,))):
        one = Call(d, p, L, flags, data_only, flip).part_read(rs)
        one.check_against_oracle()
        assert one.result() == Call(d, p, L, flags, data_only, flip).parts_read(rs).result()


def test_host_planned_shape_with_more_than_eight_rows():
    """RS(3,9) is outside the device planner; a resilver from the last three parity chunks
    rebuilds nine rows."""
    d, p = 3, 9
    rs = ce.ReedSolomon(d, p)
    for flags in ([0] * 9 + [1] * 3, [1, 0, 1] + [0, 1] + [0] * 7, [1] * 12):
        for data_only in (False, True):
            one = Call(d, p, 4099, flags, data_only).part_read(rs)
            one.check_against_oracle()
            assert one.result() == Call(d, p, 4099, flags, data_only).parts_read(rs).result()
    assert sum(1 for f in [0] * 9 + [1] * 3 if not f) > 8


def test_retry_round_passes_the_verified_chunks_on():
    d, p, L = 10, 4, 4099
    rs = ce.ReedSolomon(d, p)
    chunks, _ = _part(d, p, L)
    # round 1: chunks 1..9 good and chunk 10 (parity) damaged: d - 1 verified
    flags = [0] + [1] * d + [0] * (p - 1)
    r1 = Call(d, p, L, flags, True, flip=(d,)).part_read(rs)
    assert r1.code == ce.TOO_FEW_SHARDS_PRESENT
    assert list(r1.verified) == [0] + [1] * (d - 1) + [0] * p
    assert [bytes(s) for s in r1.slots] == r1.held  # no slot is written
    # round 2: those flagged CEC_PRESENT_VERIFIED, plus one new chunk
    flags = [0] + [VERIFIED] * (d - 1) + [0, 1] + [0] * (p - 2)
    r2 = Call(d, p, L, flags, True).part_read(rs)
    assert r2.code == ce.OK
    assert list(r2.verified) == [0] + [1] * (d - 1) + [0, 1] + [0] * (p - 2)
    assert [bytes(s) for s in r2.slots[:d]] == [chunks[i].tobytes() for i in range(d)]
    # the Python wrapper, the same two rounds
    dig = [r1.expected[32 * i:32 * (i + 1)] for i in range(d + p)]
    row = [None] + [chunks[i].tobytes() for i in range(1, d)] + [bytes(r1.held[d])] + [None] * (p - 1)
    out, ver, st = ce.part_read(rs, row, dig)
    assert st == ce.TOO_FEW_SHARDS_PRESENT and list(ver) == [0] + [1] * (d - 1) + [0] * p
    row = [None] + [(chunks[i].tobytes(), VERIFIED) for i in range(1, d)] + \
        [None, chunks[d + 1].tobytes()] + [None] * (p - 2)
    out, ver, st = ce.part_read(rs, row, dig)
    assert st == ce.OK and out[:d] == [chunks[i].tobytes() for i in range(d)]


def _damage(i, d, p):
    """(flags, flip) of caller i: erased, corrupted, trusted, too few, intact."""
    t = d + p
    flags = [1] * t
    kind = i % 6
    if kind == 0:    # erased data and parity
        flags[i % d] = 0
        flags[d + i % p] = 0
        return flags, ()
    if kind == 1:    # a corrupted copy of a data chunk
        return flags, (i % d,)
    if kind == 2:    # a retry round: d - 1 trusted, one fresh, the rest absent
        flags = [VERIFIED] * (d - 1) + [0] * (p + 1)
        flags[d + 1] = 1
        return flags, ()
    if kind == 3:    # too few: p + 1 absent
        for j in range(p + 1):
            flags[(i + j) % t] = 0
        return flags, ()
    if kind == 4:    # too few through damage: d - 1 good, two corrupted
        flags = [1] * (d + 1) + [0] * (p - 1)
        return flags, (0, d)
    return flags, ()  # intact


def test_concurrent_callers_of_mixed_lengths_and_damage_share_launches():
    d, p = 10, 4
    rs = ce.ReedSolomon(d, p)
    lens = [1, 15, 16, 17, 4096, 4099, 65539] + [65541 + 3 * i for i in range(21)] + \
        [4100 + 257 * i for i in range(20)]
    n = len(lens)
    assert n == 48
    want, calls = [], []
    for i, L in enumerate(lens):
        flags, flip = _damage(i, d, p)
        single = Call(d, p, L, flags, True, flip).part_read(rs)
        single.check_against_oracle()
        want.append(single.result())
        calls.append(Call(d, p, L, flags, True, flip))
    assert {w[0] for w in want} == {ce.OK, ce.TOO_FEW_SHARDS_PRESENT}
    barrier = threading.Barrier(n)

    def work(i):
        barrier.wait()
        calls[i].part_read(rs)

    _, c0, l0 = ce.coalesce_detail()
    threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    _, c1, l1 = ce.coalesce_detail()
    for i in range(n):
        assert calls[i].result() == want[i], (i, lens[i])
    print(f"{c1 - c0} cec_part_read calls, {l1 - l0} launches")
    assert c1 - c0 == 48 and l1 - l0 < 48
