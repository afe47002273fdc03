"""Ragged read with a packed return on the GPU: cec_read_ragged_packed_async, whose
return_plan_kernel and gather_rebuilt_kernel (csrc/plan_kernels.hip) gather every chunk the
rebuild wrote into one dense device region in part order.

The reference is cec_read_ragged_async on a second copy of the same buffer: `base`, the flags and
the statuses must be identical, every returned chunk must equal the CPU oracle's original over
exactly L bytes, the offsets must equal the host's prefix sum of n_out * stride(L), and the 0xA5
canaries before the region and from the total to the end of the allocation must be untouched.
Integer work: every comparison is exact."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import chunky_ec as ce  # noqa: E402  (after torch: one HIP runtime)
from test_gpu_ragged import LENGTHS  # noqa: E402
from test_gpu_ragged_read import CANARY, VERIFIED, _oracle_parts, _stride  # noqa: E402
from test_gpu_ragged_read_async import FILL, Case  # noqa: E402

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda", 0)
GUARD = 256  # canary bytes on either side of the return region
SHAPES = [(1, 1), (3, 2), (10, 4), (5, 5), (17, 3), (20, 8)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(d, p, data_only):
    return min(p, d) if data_only else p


def _worst(d, p, data_only, lens):
    return sum(_rows(d, p, data_only) * _stride(L) for L in lens)


class Packed:
    """One cec_read_ragged_packed_async call over a Case's batch, on a second copy of its buffer,
    with a canary-framed return region of `cap` bytes (default: the worst case)."""

    def __init__(self, case, cap=None, slack=0):
        c = self.c = case
        d = c.rs.data_shard_count()
        self.data_only = not c.resilver
        self.cap = _worst(d, c.t - d, self.data_only, c.lens) if cap is None else cap
        self.buf = torch.from_numpy(c.before).to(DEV)
        self.region = torch.full((GUARD + self.cap + slack + GUARD,), CANARY, dtype=torch.uint8,
                                 device=DEV)
        assert (self.region.data_ptr() + GUARD) % 16 == 0
        self.ver = ce.HostBuffer(c.n * c.t)
        self.st = ce.HostBuffer(c.n * 4)
        self.off = ce.HostBuffer((c.n + 1) * 8)
        for b in (self.ver, self.st, self.off):
            b.array[:] = FILL
        torch.cuda.synchronize()

    def queue(self, stream=None):
        c = self.c
        ce.read_ragged_packed_async(c.rs, self.buf.data_ptr(), c.offs, c.lens, c.flags.tobytes(),
                                    c.dexp.data_ptr(), self.data_only, self.ver, self.st,
                                    self.region.data_ptr() + GUARD, self.cap, self.off, stream)

    def untouched(self):
        return all(bool((b.array == FILL).all()) for b in (self.ver, self.st, self.off)) and \
            bool((self.region == CANARY).all()) and \
            np.array_equal(self.buf.cpu().numpy(), self.c.before)

    def offsets(self):
        return self.off.array.view(np.uint64).astype(np.int64)

    def check(self):
        """After both calls' work is done: everything the module docstring lists."""
        c = self.c
        d = c.rs.data_shard_count()
        c.check()  # the reference call against the oracle
        assert np.array_equal(self.buf.cpu().numpy(), c.buf.cpu().numpy()), "base differs"
        assert np.array_equal(self.ver.array, c.ver.array), "verified differs"
        assert np.array_equal(self.st.array, c.st.array), "part_status differs"
        ver, st = c.ver.array.reshape(c.n, c.t), c.statuses()
        fill = np.ones(c.t, bool) if c.resilver else np.arange(c.t) < d
        n_out = np.where(st == ce.OK, ((ver == 0) & fill).sum(axis=1), 0)
        strides = np.array([_stride(L) for L in c.lens], np.int64)
        want_off = np.concatenate([[0], np.cumsum(n_out * strides)])
        got_off = self.offsets()
        assert np.array_equal(got_off, want_off), \
            f"offsets differ first at part {np.flatnonzero(got_off != want_off)[:1]}"
        total = int(want_off[-1])
        assert total <= self.cap
        region = self.region.cpu().numpy()
        assert (region[:GUARD] == CANARY).all(), "a byte before the region was written"
        assert (region[GUARD + total:] == CANARY).all(), "a byte at or behind the total was written"
        ret = region[GUARD:GUARD + total]
        for k in np.flatnonzero(n_out):
            L, cs, r = c.lens[k], int(strides[k]), 0
            for i in np.flatnonzero((ver[k] == 0) & fill):
                at = int(want_off[k]) + r * cs
                assert np.array_equal(ret[at:at + L], c.parts[k][0][i]), (k, i)
                r += 1
            assert r == n_out[k]
        return n_out, total


def _run(case, **kw):
    c = case.upload()
    pk = Packed(c, **kw)
    c.queue()
    pk.queue()
    torch.cuda.synchronize()
    return pk, pk.check()


# ----------------------------------------------------------------------------------------------
# 1. one part per length, every shape and mode
# ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_batches():
    """One batch per shape, one part per chunk length: computed once, shared, never modified."""
    return {(d, p): _oracle_parts(d, p, LENGTHS, 10 * d + p) for d, p in SHAPES}


def _mixed(d, p, data_only, n):
    """flags [n][t] and the flipped chunk: part k misses k % (rows + 1) of the slots the mode
    fills (seeded places); one part misses p + 1 chunks (undecodable), one with nothing missing
    has its loaded data chunk 0 flipped, one has a loaded chunk flagged PRESENT_VERIFIED."""
    t, rows = d + p, _rows(d, p, data_only)
    rng = np.random.default_rng(1000 * d + 10 * p + data_only)
    fillable = d if data_only else t
    flags = np.ones((n, t), np.uint8)
    for k in range(n):
        flags[k, rng.permutation(fillable)[:k % (rows + 1)]] = 0
    undecodable, corrupt, trusted = 5, 2 * (rows + 1), 7
    assert len({undecodable, corrupt, trusted}) == 3 and corrupt < n
    flags[undecodable] = 1
    flags[undecodable, rng.permutation(t)[:p + 1]] = 0
    assert flags[corrupt].all()
    flags[trusted, np.flatnonzero(flags[trusted])[-1]] = VERIFIED
    return flags, {(corrupt, 0)}, undecodable


@pytest.mark.parametrize("data_only", [1, 0], ids=["data_only", "all"])
@pytest.mark.parametrize("d,p", SHAPES)
def test_packed_return_equals_the_async_call_and_the_oracle(d, p, data_only, oracle_batches):
    parts = oracle_batches[(d, p)]
    rows = _rows(d, p, data_only)
    flags, flip, undecodable = _mixed(d, p, data_only, len(parts))
    case = Case(ce.ReedSolomon(d, p), parts, flags, not data_only, flip=flip)
    pk, (n_out, total) = _run(case)
    st = case.statuses()
    assert st[undecodable] == ce.TOO_FEW_SHARDS_PRESENT and n_out[undecodable] == 0
    assert (np.delete(st, undecodable) == ce.OK).all()
    (ck, ci), = flip
    assert case.ver.array[ck * (d + p) + ci] == 0 and n_out[ck] == 1  # rebuilt and returned
    assert set(n_out) == set(range(rows + 1)) and total > 0


# ----------------------------------------------------------------------------------------------
# 2. the scan's boundaries
# ----------------------------------------------------------------------------------------------

def _scan_block():
    src = open(os.path.join(ROOT, "chunky-bits_amd", "csrc", "plan_kernels.hip")).read()
    return int(re.search(r"constexpr uint32_t kRetThreads = (\d+);", src).group(1))


B = _scan_block()
SCAN_N = [1, 63, 64, 65, B - 1, B, B + 1, 4 * B + 1, 4096]


@pytest.fixture(scope="module")
def tiny_parts():
    """4096 RS(3,2) parts of 1..17 bytes per chunk; the smaller batches are prefixes."""
    return _oracle_parts(3, 2, [1 + k % 17 for k in range(max(SCAN_N))], 77)


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_boundaries(n, tiny_parts):
    d, p = 3, 2
    rng = np.random.default_rng(n)
    flags = np.ones((n, d + p), np.uint8)
    for k in range(n):
        gone = 3 if k % 7 == 6 else k % 3  # every 7th part cannot be decoded
        flags[k, rng.permutation(d + p)[:gone]] = 0
    case = Case(ce.ReedSolomon(d, p), tiny_parts[:n], flags, True)
    pk, (n_out, total) = _run(case)
    want = [0 if k % 7 == 6 else k % 3 for k in range(n)]
    assert list(n_out) == want
    assert total == sum(r * _stride(L) for r, L in zip(want, case.lens))


# ----------------------------------------------------------------------------------------------
# 3. nothing to return, and the refusals
# ----------------------------------------------------------------------------------------------

def test_nothing_to_rebuild_returns_nothing(oracle_batches):
    d, p = 3, 2
    parts = oracle_batches[(d, p)]
    flags = np.ones((len(parts), d + p), np.uint8)
    pk, (n_out, total) = _run(Case(ce.ReedSolomon(d, p), parts, flags, True))
    assert total == 0 and not n_out.any()
    assert bool((pk.region == CANARY).all())


@pytest.mark.parametrize("data_only", [1, 0], ids=["data_only", "all"])
def test_cap_one_column_under_the_worst_case_is_refused(data_only, oracle_batches):
    d, p = 10, 4
    parts = oracle_batches[(d, p)]
    flags = np.ones((len(parts), d + p), np.uint8)
    flags[:, 0] = 0
    case = Case(ce.ReedSolomon(d, p), parts, flags, not data_only).upload()
    worst = _worst(d, p, data_only, case.lens)
    pk = Packed(case, cap=worst - 16, slack=16)
    with pytest.raises(ce.Error) as e:
        pk.queue()
    torch.cuda.synchronize()
    assert e.value.code == ce.ERR_INVALID_ARGUMENT and "rebuilt_cap" in str(e.value)
    assert pk.untouched()  # nothing was queued
    pk = Packed(case, cap=worst)  # and the worst case itself is enough
    case.queue()
    pk.queue()
    torch.cuda.synchronize()
    pk.check()


def test_a_shape_outside_the_planner_is_refused():
    d, p = 4, 9
    parts = _oracle_parts(d, p, [1, 17, 4097], 3)
    flags = np.ones((3, d + p), np.uint8)
    flags[:, 1] = 0
    case = Case(ce.ReedSolomon(d, p), parts, flags, False).upload()
    pk = Packed(case)
    with pytest.raises(ce.Error) as e:
        pk.queue()
    torch.cuda.synchronize()
    assert e.value.code == ce.ERR_INVALID_ARGUMENT and "planner" in str(e.value)
    assert pk.untouched()
