"""Small files through the write path's compute: per-part calls against one ragged batch.

Host-staged workload (default): files from seed 1, sizes log-uniform in [1 KiB, 4 MiB], 4096 of
them (about 2 GiB), cut into parts of d x 1 MiB as FileWriteBuilder does, for RS(3,2) and
RS(10,4).  Three arms produce the same parts:

  a  the per-part way: cec_part_encode per part from 10 and from 256 threads (the padded copy of
     each part that call needs is made before the clock starts), each with CEC_COALESCE_MIXED 0
     (one chunk length per coalesced batch) and 1 (any lengths together); --per-part-only runs
     these arms alone
  b  one cec_parts_encode call over all parts, straight from the files' bytes
  c  the CPU oracle (the crate's path restated in C) on 16 threads
  d  the parts pipeline: cec_parts_pipeline_submit_from per slot-sized batch of consecutive
     parts, straight from the files' bytes, one arm per --depths entry (3 and 2 slots in flight
     by default, --slot-mib of data each; --no-per-part leaves the a arms out); the oldest
     slot is collected while the later ones run.  The digests are copied out; the parity stays in
     the slot's pinned region, where FileWriteBuilder reads it (compared with b's once, untimed)

Every arm is warmed up, then the arms alternate three times in one process; the device is
synchronised before each clock reading.  Reported: GB/s of file bytes and parts/s per repeat.
All arms' digests must agree (asserted).

--segment BYTES[,BYTES...]: the same files and shapes through three arms that alternate: (a) the one
cec_parts_encode call (arm b above), (b) the parts pipeline (arm d above, one arm per --depths
entry) and (c) the segment pipeline, cec_segment_pipeline_submit_from, one arm per segment size
and --depths entry: a part whose chunks are longer than the segment goes as column segments, one
per batch, each batch first taking the next segment of every open part (--max-open at most;
default: as many as a slot holds segments) and then new parts while the slot lasts (the plan is made before the clock starts, as for b).  The digests of
the entries that end a part are copied out; the parity stays in the slots (put together and
compared with a's once, untimed).  All arms' digests must agree (asserted).  A segment arm counts
as faster than an incumbent only if its worst repeat is below the incumbent's best, and a switch
of a default needs that at both shapes.

--device: 4096 x RS(10,4) x 64 KiB parts, device resident: cec_encode_hash_ragged with uniform
lengths, by its two-pass path (CEC_RAGGED_FUSED=0) and by the fused kernel (=1), and
cec_encode_hash_split (the same parts, data and parity in regions of their own) against
cec_encode_hash_batch on the same bytes; the times and the ratios.  Then the files of the
host-staged workload as packed device-resident parts at RS(3,2) and at RS(10,4): one
cec_encode_hash_ragged call by either path.  Arms alternate after a warm-up, each call timed
between two stream events; all arms' parity and digests must be equal (asserted).  The fused
kernel becomes the default for large ragged launches only if its worst repeat is below the
two-pass path's best in all three configurations.

--read: the read side on the same seeded files and shapes.  Every part is stored as the oracle
encodes it and its data chunk k % d is erased, so every part is decoded from d - 1 data chunks and
the first parity chunk:

  a  the per-part way from 10 and from 256 threads: cec_sha256_many over the d loaded chunks,
     the digests compared, then cec_reconstruct_data; and the same in one call per part,
     cec_part_read
  b  one cec_parts_read call over all parts
  c  the CPU oracle on 16 threads (SHA-256 of the d loaded chunks, reconstruct_data)
  d  the parts reader: cec_parts_reader_submit_from per slot-sized batch of consecutive parts
     (--slot-mib of ragged layout each), one arm per --depths entry; the oldest slot is waited
     for and scattered into the same output slots while the later ones run

All arms' rebuilt chunks must equal the erased ones (asserted).  Beside the times, the bytes
each of b and d brings back from the device per pass: d's from cec_parts_reader_stats, b's the
copies its copy_spans step issues (rebuilt spans merged across gaps under 256 KiB, per round of
CEC_COALESCE_MAX_MIB), counted here from the same layout.  d counts as faster than b only if its
worst repeat is below b's best by more than the larger spread of the two.

--device --read: 4096 x RS(10,4) x 64 KiB, two erasures per part, device resident:
cec_reconstruct_ragged with uniform lengths against cec_reconstruct_batch on the same bytes.
Then cec_read_ragged against cec_read_ragged_async (the decode planned on the device, no wait in
the call) on that batch and on the seeded files as device-resident RS(10,4) and RS(3,2) parts
with one data chunk per part erased: (a) one call over all parts, the interval between two stream
events and the host's time inside the call; (b) the parts in two halves on two streams from one
thread, wall time to the second synchronise.  Arms alternate after a warm-up; the rebuilt bytes,
flags and statuses must be equal between the arms (asserted).  The async form counts as a gain
in (b) only if its worst repeat is below the synchronous form's best.

--verify: the scrub side on the same seeded files and shapes.  Every part is stored as the oracle
encodes it and every one of its d + p chunks is hashed and compared with its digest:

  a  the per-part way from 10 and from 256 threads: cec_sha256_many over the part's d + p chunks,
     the digests compared (FilePart::verify)
  b  one cec_parts_verify call over all chunks of all parts
  c  the CPU oracle on 16 threads (SHA-256 of every chunk, compared)

Every arm must find every chunk good, and the one chunk that is flipped before the run bad
(asserted).

--verify --segment BYTES[,BYTES...]: the same copies, one in 97 of them damaged (its first, a
middle or its last byte), through two arms that alternate three times after a warm-up: (a) the one
cec_parts_verify call (arm b above) and (c) the scrub pipeline, cec_scrub_pipeline_submit_from,
one arm per segment size and --depths entry: a copy longer than the segment goes as segments, one
per batch, each batch first taking the next segment of every open copy (--max-open at most;
default: as many as a slot holds segments) and then new copies while the slot lasts (the plan, the
pointer tables and the expected rows are made before the clock starts).  The flags of the entries
that end a copy are copied out.  Every arm's flags must equal arm a's and the damage done
(asserted).  Reported: GB/s of copy bytes per repeat, the batches and the most copies open; arm c
counts as faster only if its worst repeat is above arm a's best.

    python tools/small_files_bench.py [--files 4096] [--repeats 3] [--shapes 3,2:10,4]
                                      [--slot-mib 64] [--depths 3,2] [--no-per-part]
    python tools/small_files_bench.py --segment 16384,65536,262144 [--slot-mib 64] [--depths 3,2]
    python tools/small_files_bench.py --device
    python tools/small_files_bench.py --read [--slot-mib 64] [--depths 3,2] [--no-per-part]
    python tools/small_files_bench.py --verify
    python tools/small_files_bench.py --verify --segment 16384,65536 [--slot-mib 64] [--depths 3,2]
    python tools/small_files_bench.py --device --read"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "chunky-bits_amd"))
import torch  # noqa: E402
import chunky_ec as ce  # noqa: E402
import oracle  # noqa: E402

CHUNK = 1 << 20
U8P = ctypes.POINTER(ctypes.c_uint8)


def make_files(n_files, seed=1):
    """(pool, [(offset, size)]): file f is pool[offset : offset + size]."""
    rng = np.random.default_rng(seed)
    sizes = np.exp(rng.uniform(np.log(1 << 10), np.log(4 << 20), n_files)).astype(np.int64)
    pool = rng.integers(0, 256, (64 << 20) + (4 << 20), dtype=np.uint8)
    offs = rng.integers(0, 64 << 20, n_files)
    return pool, [(int(o), int(s)) for o, s in zip(offs, sizes)]


def cut_parts(files, d):
    """Every file's parts, in file order: (offset into the pool, length)."""
    cap = d * CHUNK
    parts = []
    for off, size in files:
        for at in range(0, size, cap):
            parts.append((off + at, min(cap, size - at)))
    return parts


class Workload:
    def __init__(self, pool, files, d, p):
        self.d, self.p, self.t = d, p, d + p
        self.rs = ce.ReedSolomon(d, p)
        self.pool = pool
        self.parts = cut_parts(files, d)
        self.n = len(self.parts)
        self.file_bytes = sum(s for _, s in files)
        self.L = [(ln + d - 1) // d for _, ln in self.parts]
        base = pool.ctypes.data
        self.ptrs = (U8P * self.n)(*[ctypes.cast(base + o, U8P) for o, _ in self.parts])
        self.lens = (ctypes.c_size_t * self.n)(*[ln for _, ln in self.parts])
        # outputs (reused by every arm and repeat)
        self.par_off = np.concatenate([[0], np.cumsum([p * L for L in self.L])])
        self.parity = np.zeros(int(self.par_off[-1]), np.uint8)
        pb = self.parity.ctypes.data
        self.par_ptrs = (U8P * self.n)(*[ctypes.cast(pb + int(o), U8P)
                                         for o in self.par_off[:-1]])
        self.chunksizes = (ctypes.c_size_t * self.n)()
        # arm a / c input: each part zero padded to d * L (the copy cec_part_encode's callers make)
        self.pad_off = np.concatenate([[0], np.cumsum([d * L for L in self.L])])
        self.padded = np.zeros(int(self.pad_off[-1]), np.uint8)
        for k, (o, ln) in enumerate(self.parts):
            at = int(self.pad_off[k])
            self.padded[at:at + ln] = pool[o:o + ln]

    def digests(self):
        return np.zeros((self.n, self.t, 32), np.uint8)

    def _one(self, fn, dig, k):
        cs = ctypes.c_size_t(0)
        src = ctypes.cast(self.padded.ctypes.data + int(self.pad_off[k]), U8P)
        par = ctypes.cast(self.parity.ctypes.data + int(self.par_off[k]), U8P)
        out = ctypes.cast(dig.ctypes.data + k * self.t * 32, U8P)
        st = fn(src, self.parts[k][1], par, out, ctypes.byref(cs))
        assert st == 0 and cs.value == self.L[k], (st, k)

    def arm_percall(self, threads, count=None):
        dig = self.digests()
        h = self.rs.handle

        def fn(src, ln, par, out, cs):
            return ce._lib.cec_part_encode(h, src, ln, par, out, cs)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda k: self._one(fn, dig, k), range(count or self.n)))
        return dig

    def arm_ragged(self, count=None):
        dig = self.digests()
        ce._check(ce._lib.cec_parts_encode(self.rs.handle, self.ptrs, self.lens, count or self.n,
                                           self.par_ptrs, dig.ctypes.data_as(U8P),
                                           self.chunksizes))
        return dig

    def arm_cpu(self, threads=16, count=None):
        dig = self.digests()
        lib = oracle.lib()
        d, p = self.d, self.p

        def fn(src, ln, par, out, cs):
            return lib.or_part_encode(d, p, src, ln, par, out, cs)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda k: self._one(fn, dig, k), range(count or self.n)))
        return dig

    def make_pipeline(self, slot_bytes, depth, max_parts=4096):
        """A cec_parts_pipeline and the batches the parts fall into (consecutive parts while
        their padded data fits a slot and their count max_parts), made before any clock starts,
        as FileWriteBuilder keeps its pipeline between calls."""
        d = self.d
        slot_bytes = max(slot_bytes, d * ce.ragged_stride(CHUNK))
        pl = ce.PartsPipeline(self.rs, slot_bytes, max_parts, depth)
        batches, k0, used = [], 0, 0
        for k, L in enumerate(self.L):
            b = d * ce.ragged_stride(L)
            if k > k0 and (used + b > slot_bytes or k - k0 == max_parts):
                batches.append((k0, k))
                k0, used = k, 0
            used += b
        batches.append((k0, self.n))
        pp = ctypes.POINTER(U8P)
        szp = ctypes.POINTER(ctypes.c_size_t)
        step = ctypes.sizeof(ctypes.c_size_t)
        args = [(ctypes.cast(ctypes.addressof(self.ptrs) + a * ctypes.sizeof(U8P), pp),
                 ctypes.cast(ctypes.addressof(self.lens) + a * step, szp), b - a,
                 ctypes.cast(ctypes.addressof(self.chunksizes) + a * step, szp))
                for a, b in batches]
        return pl, batches, args

    def arm_pipeline(self, pipe, check_parity=False):
        """Every batch through the pipeline's slots with submit_from; while later slots run the
        oldest is collected: its digests copied out, its parity left in the slot's pinned region
        (where FileWriteBuilder reads it) unless check_parity compares it with self.parity."""
        pl, batches, args = pipe
        dig = self.digests()
        lib, h, t = ce._lib, pl._h, self.t
        slot, ptr, par, dg, n = (ctypes.c_size_t(0), U8P(), U8P(), U8P(), ctypes.c_size_t(0))
        pending = []

        def collect():
            s, (a, b) = pending.pop(0)
            ce._check(lib.cec_parts_pipeline_wait(h, s, ctypes.byref(par), ctypes.byref(dg),
                                                  ctypes.byref(n)))
            assert n.value == b - a
            ctypes.memmove(dig.ctypes.data + a * t * 32, dg, (b - a) * t * 32)
            if check_parity:
                _, poffs, _, pb = ce.split_layout(self.d, self.p, self.L[a:b])
                got = np.ctypeslib.as_array(par, shape=(pb,))
                for k in range(a, b):
                    L, cs = self.L[k], ce.ragged_stride(self.L[k])
                    for i in range(self.p):
                        at, to = poffs[k - a] + i * cs, int(self.par_off[k]) + i * L
                        assert np.array_equal(got[at:at + L], self.parity[to:to + L]), (k, i)
        for rng, (bufs, lens, cnt, cs) in zip(batches, args):
            if len(pending) == pl.depth:
                collect()
            ce._check(lib.cec_parts_pipeline_acquire(h, ctypes.byref(slot), ctypes.byref(ptr)))
            ce._check(lib.cec_parts_pipeline_submit_from(h, slot.value, bufs, lens, cnt, cs))
            pending.append((slot.value, rng))
        while pending:
            collect()
        return dig


    def make_segment_pipeline(self, slot_bytes, depth, segment, max_parts=4096, max_open=None):
        """A cec_segment_pipeline and the plan of its batches, made before any clock starts: each
        batch takes the next segment of every open part, in part order, then new parts while the
        slot, max_parts and the open ids last (the rule of FileWriteBuilder::many_segment).  Per
        batch: the entries (part, offset, length, last), the call's arrays, and for the entries
        that end a part their rows and parts."""
        d = self.d
        slot_bytes = max(slot_bytes, d * ce.ragged_stride(CHUNK))
        if not max_open:  # as many open parts as a slot holds segments (many_segment's default)
            max_open = max(1, min(max_parts, slot_bytes // (d * ce.ragged_stride(segment))))
        pl = ce.SegmentPipeline(self.rs, slot_bytes, max_parts, depth, max_open)
        free, open_parts, nxt, plan = list(range(max_open))[::-1], [], 0, []
        while nxt < self.n or open_parts:
            batch, room, still, freed = [], slot_bytes, [], []

            def fits(ln):
                return len(batch) < max_parts and d * ce.ragged_stride(ln) <= room
            for k, done, oid in open_parts:
                ln = min(segment, self.L[k] - done)
                if not fits(ln):
                    still.append((k, done, oid))
                    continue
                batch.append((k, done, ln, oid))
                room -= d * ce.ragged_stride(ln)
                if done + ln == self.L[k]:
                    freed.append(oid)
                else:
                    still.append((k, done + ln, oid))
            while nxt < self.n:
                ln = min(segment, self.L[nxt])
                whole = ln == self.L[nxt]
                if not fits(ln) or (not whole and not free):
                    break
                oid = 0 if whole else free.pop()
                if not whole:
                    still.append((nxt, ln, oid))
                batch.append((nxt, 0, ln, oid))
                room -= d * ce.ragged_stride(ln)
                nxt += 1
            free += freed
            open_parts = still
            m = len(batch)
            last = [q for q, (k, off, ln, _) in enumerate(batch) if off + ln == self.L[k]]
            plan.append({
                "entries": batch,
                "bufs": (U8P * m)(*[self.ptrs[k] for k, _, _, _ in batch]),
                "lengths": (ctypes.c_size_t * m)(*[self.lens[k] for k, _, _, _ in batch]),
                "offs": (ctypes.c_size_t * m)(*[e[1] for e in batch]),
                "segs": (ctypes.c_size_t * m)(*[e[2] for e in batch]),
                "ids": (ctypes.c_uint32 * m)(*[e[3] for e in batch]),
                "cs": (ctypes.c_size_t * m)(),
                "last_rows": np.array(last, np.int64),
                "last_parts": np.array([batch[q][0] for q in last], np.int64)})
        return pl, plan

    def arm_segments(self, pipe, check_parity=False):
        """Every planned batch through the segment pipeline's slots; while later slots run the
        oldest is collected: the digests of the entries that end a part copied out, the parity
        pieces left in the slot's pinned region unless check_parity puts them together and
        compares them with self.parity."""
        pl, plan = pipe
        dig = self.digests()
        lib, h, t = ce._lib, pl._h, self.t
        slot, par, dg, n = ctypes.c_size_t(0), U8P(), U8P(), ctypes.c_size_t(0)
        pending = []
        got_par = np.zeros_like(self.parity) if check_parity else None

        def collect():
            s, b = pending.pop(0)
            ce._check(lib.cec_segment_pipeline_wait(h, s, ctypes.byref(par), ctypes.byref(dg),
                                                    ctypes.byref(n)))
            m = len(b["entries"])
            assert n.value == m
            rows = np.ctypeslib.as_array(dg, shape=(m, t, 32))
            dig[b["last_parts"]] = rows[b["last_rows"]]
            if check_parity:
                _, poffs, _, pb = ce.split_layout(self.d, self.p, [e[2] for e in b["entries"]])
                got = np.ctypeslib.as_array(par, shape=(pb,))
                for (k, off, ln, _), po in zip(b["entries"], poffs):
                    cs = ce.ragged_stride(ln)
                    for i in range(self.p):
                        to = int(self.par_off[k]) + i * self.L[k] + off
                        got_par[to:to + ln] = got[po + i * cs:po + i * cs + ln]
        for b in plan:
            if len(pending) == pl.depth:
                collect()
            ce._check(lib.cec_segment_pipeline_acquire(h, ctypes.byref(slot)))
            ce._check(lib.cec_segment_pipeline_submit_from(
                h, slot.value, b["bufs"], b["lengths"], b["offs"], b["segs"], b["ids"],
                len(b["entries"]), b["cs"]))
            pending.append((slot.value, b))
        while pending:
            collect()
        assert pl.open_count() == 0
        if check_parity:
            assert np.array_equal(got_par, self.parity), "assembled parity differs from a's"
        return dig


def set_env_knob(name, value):
    """CEC_* knob `name` = value (None: unset) from the next call on."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    ce.reload_knobs()


MIXED = "CEC_COALESCE_MIXED"


def with_mixed(value, fn):
    """fn() with CEC_COALESCE_MIXED = value, the knob restored behind it."""
    before = os.environ.get(MIXED)
    set_env_knob(MIXED, value)
    try:
        return fn()
    finally:
        set_env_knob(MIXED, before)


def mixed_verdict(secs, threads, row):
    """The rule of DESIGN.md 4.6 for one thread count: mixed gathering's worst repeat against the
    by-length arm's best."""
    by_len = secs[f"a: part_encode x {threads} threads, by length"]
    mixed = secs[f"a: part_encode x {threads} threads, mixed"]
    wins = max(mixed) < min(by_len)
    row[f"mixed_vs_by_length_{threads}"] = {"by_length_best_s": min(by_len),
                                            "mixed_worst_s": max(mixed), "mixed_wins": wins}
    print(f"   mixed vs by length, {threads} threads: by length {min(by_len):.3f}-{max(by_len):.3f} s, "
          f"mixed {min(mixed):.3f}-{max(mixed):.3f} s -> mixed's worst beats by-length's best: {wins}",
          flush=True)
    return wins


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def host_staged(args):
    pool, files = make_files(args.files)
    results = []
    for shape in args.shapes.split(":"):
        d, p = (int(x) for x in shape.split(","))
        w = Workload(pool, files, d, p)
        print(f"== RS({d},{p}) chunk 1 MiB: {len(files)} files, {w.file_bytes / 2**30:.2f} GiB, "
              f"{w.n} parts, {len(set(w.L))} distinct chunk lengths", flush=True)
        # the per-part arms under both values of CEC_COALESCE_MIXED, alternating
        arms = [(f"a: part_encode x {th} threads, {how}",
                 lambda c=None, th=th, knob=knob: with_mixed(knob, lambda: w.arm_percall(th, c)))
                for th in (10, 256) for knob, how in (("0", "by length"), ("1", "mixed"))]
        arms += [("b: one parts_encode call", lambda c=None: w.arm_ragged(c)),
                 ("c: CPU oracle x 16 threads", lambda c=None: w.arm_cpu(16, c))]
        slot = args.slot_mib << 20
        if args.no_per_part:  # a quick look at arm d: the per-part arms take most of a run
            arms = [arm for arm in arms if not arm[0].startswith("a")]
        if args.per_part_only:  # the A/B of the per-part arms alone
            arms = [arm for arm in arms if arm[0].startswith("a")]
            args.depths = []
        pipes = {depth: w.make_pipeline(slot, depth) for depth in args.depths}
        d_names = {depth: f"d: parts pipeline (submit_from) {args.slot_mib} MiB x {depth}"
                   for depth in pipes}
        for depth, pipe in pipes.items():
            arms.append((d_names[depth], lambda c=None, pipe=pipe: w.arm_pipeline(pipe)))
        warm = min(w.n, 512)
        for name, fn in arms:  # warm-up: b and d on the whole input (b's staging is sized by it)
            sec, _ = timed(lambda: fn(None if name[0] in "bd" else warm))
            print(f"   warm-up {name}: {sec:.3f} s", flush=True)
        for depth, pipe in pipes.items():  # d's parity, left in the slots, against b's (untimed)
            w.arm_pipeline(pipe, check_parity=True)
        if pipes:
            print(f"   d: {len(pipes[args.depths[0]][1])} batches; parity in the slots equals "
                  f"b's", flush=True)
        secs = {name: [] for name, _ in arms}
        ref = None
        for rep in range(args.repeats):
            for name, fn in arms:
                sec, dig = timed(fn)
                secs[name].append(sec)
                if ref is None:
                    ref = dig
                assert np.array_equal(dig, ref), f"digests of '{name}' differ"
                print(f"   repeat {rep + 1} {name}: {sec:.3f} s  "
                      f"{w.file_bytes / sec / 1e9:7.2f} GB/s  {w.n / sec:9.0f} parts/s", flush=True)
        hl = [h.hex() for h in (ref[0, 0].tobytes(), ref[-1, -1].tobytes())]
        print(f"   digests agree across all arms and repeats (first {hl[0][:16]}, "
              f"last {hl[1][:16]})")
        row = {"d": d, "p": p, "files": len(files), "parts": w.n, "file_bytes": w.file_bytes,
               "seconds": secs,
               "gbps": {k: [w.file_bytes / s / 1e9 for s in v] for k, v in secs.items()}}
        if not args.no_per_part:
            row["mixed_wins"] = [mixed_verdict(secs, th, row) for th in (10, 256)]
        b = secs.get("b: one parts_encode call")
        if not args.no_per_part and b:
            a = min(secs["a: part_encode x 256 threads, by length"],
                    secs["a: part_encode x 256 threads, mixed"], key=min)
            spread = max(max(a) - min(a), max(b) - min(b))
            row["b_vs_a256"] = {"a_best_s": min(a), "b_worst_s": max(b), "spread_s": spread,
                                "b_wins_by_more_than_spread": max(b) + spread < min(a)}
            print(f"   b vs a(256): a best {min(a):.3f} s, b worst {max(b):.3f} s, largest spread "
                  f"{spread:.3f} s -> b wins by more than the spread: "
                  f"{row['b_vs_a256']['b_wins_by_more_than_spread']}", flush=True)
        for depth, name in d_names.items():  # the same rule for the pipeline against b
            dd = secs[name]
            spread = max(max(dd) - min(dd), max(b) - min(b))
            wins = max(dd) + spread < min(b)
            row[f"d{depth}_vs_b"] = {"b_best_s": min(b), "d_worst_s": max(dd), "spread_s": spread,
                                     "d_wins_by_more_than_spread": wins}
            print(f"   d (depth {depth}) vs b: b best {min(b):.3f} s, d worst {max(dd):.3f} s, "
                  f"largest spread {spread:.3f} s -> d wins by more than the spread: {wins}",
                  flush=True)
        results.append(row)
        del w, pipes
    print(json.dumps({"tool": "small_files_bench", "mode": "host", "results": results}))


def host_segments(args):
    """--segment: the one call, the parts pipeline and the segment pipeline, alternating."""
    pool, files = make_files(args.files)
    results = []
    slot = args.slot_mib << 20
    for shape in args.shapes.split(":"):
        d, p = (int(x) for x in shape.split(","))
        w = Workload(pool, files, d, p)
        print(f"== RS({d},{p}) chunk 1 MiB: {len(files)} files, {w.file_bytes / 2**30:.2f} GiB, "
              f"{w.n} parts, longest chunk {max(w.L)} bytes", flush=True)
        arms = [("a: one parts_encode call", w.arm_ragged)]
        for depth in args.depths:
            pipe = w.make_pipeline(slot, depth)
            arms.append((f"b: parts pipeline {args.slot_mib} MiB x {depth}",
                         lambda pipe=pipe: w.arm_pipeline(pipe)))
        seg_pipes = {}
        for seg in args.segment:
            for depth in args.depths:
                size = f"{seg >> 10} KiB" if seg % 1024 == 0 else f"{seg} B"
                name = f"c: segment pipeline {size} segments, {args.slot_mib} MiB x {depth}"
                seg_pipes[name] = w.make_segment_pipeline(slot, depth, seg,
                                                          max_open=args.max_open)
                arms.append((name, lambda pipe=seg_pipes[name]: w.arm_segments(pipe)))
                print(f"   {name}: {len(seg_pipes[name][1])} batches, up to "
                      f"{seg_pipes[name][0].max_open} parts open", flush=True)
        for name, fn in arms:
            sec, _ = timed(fn)
            print(f"   warm-up {name}: {sec:.3f} s", flush=True)
        for name, pipe in seg_pipes.items():  # c's parity against a's (untimed)
            w.arm_segments(pipe, check_parity=True)
        print("   c: the parity pieces in the slots, put together, equal a's parity", flush=True)
        secs = {name: [] for name, _ in arms}
        ref = None
        for rep in range(args.repeats):
            for name, fn in arms:
                sec, dig = timed(fn)
                secs[name].append(sec)
                if ref is None:
                    ref = dig
                assert np.array_equal(dig, ref), f"digests of '{name}' differ"
                print(f"   repeat {rep + 1} {name}: {sec:.3f} s  "
                      f"{w.file_bytes / sec / 1e9:7.2f} GB/s", flush=True)
        print("   digests agree across all arms and repeats")
        gbps = {k: [w.file_bytes / x / 1e9 for x in v] for k, v in secs.items()}
        row = {"d": d, "p": p, "files": len(files), "parts": w.n, "file_bytes": w.file_bytes,
               "seconds": secs, "gbps": gbps, "verdicts": {}}
        for name in seg_pipes:
            for inc in [n for n, _ in arms if n[0] in "ab"]:
                wins = min(gbps[name]) > max(gbps[inc])
                row["verdicts"][f"{name} over {inc}"] = wins
                print(f"   {name}: {min(gbps[name]):.2f}-{max(gbps[name]):.2f} GB/s against "
                      f"{inc}: {min(gbps[inc]):.2f}-{max(gbps[inc]):.2f} GB/s -> worst above the "
                      f"incumbent's best: {wins}", flush=True)
        results.append(row)
        del w, seg_pipes, arms
    print(json.dumps({"tool": "small_files_bench", "mode": "segment", "results": results}))


def oracle_store(pool, parts, L, d, p):
    """The parts as the oracle stores them -> (off, store, expected): part k's d + p chunks of
    L[k] bytes from store[off[k]], its digests in expected[k]."""
    n, t = len(parts), d + p
    off = np.concatenate([[0], np.cumsum([t * x for x in L])])
    store = np.zeros(int(off[-1]), np.uint8)
    expected = np.zeros((n, t, 32), np.uint8)
    lib = oracle.lib()
    sb, eb = store.ctypes.data, expected.ctypes.data

    def encode(k):
        o, ln = parts[k]
        at = int(off[k])
        store[at:at + ln] = pool[o:o + ln]
        cs = ctypes.c_size_t(0)
        st = lib.or_part_encode(d, p, ctypes.cast(sb + at, U8P), ln,
                                ctypes.cast(sb + at + d * L[k], U8P),
                                ctypes.cast(eb + k * t * 32, U8P), ctypes.byref(cs))
        assert st == 0 and cs.value == L[k]
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(encode, range(n)))
    return off, store, expected


class ReadWorkload:
    """The parts of `files` as the oracle stores them (d data + p parity chunks of L_k bytes,
    digests), data chunk k % d of part k erased; d - 1 data chunks and parity chunk 0 are loaded."""

    def __init__(self, pool, files, d, p):
        self.d, self.p, self.t = d, p, d + p
        self.rs = ce.ReedSolomon(d, p)
        self.parts = cut_parts(files, d)
        self.n = n = len(self.parts)
        self.file_bytes = sum(s for _, s in files)
        self.L = [(ln + d - 1) // d for _, ln in self.parts]
        t = self.t
        self.off, self.store, self.expected = oracle_store(pool, self.parts, self.L, d, p)
        sb = self.store.ctypes.data
        self.erased = [k % d for k in range(n)]
        self.loaded = [[i for i in range(d) if i != self.erased[k]] + [d] for k in range(n)]
        # the erased chunks, kept aside and wiped in the store
        self.out_off = np.concatenate([[0], np.cumsum(self.L)])
        self.want = np.zeros(int(self.out_off[-1]), np.uint8)
        for k in range(n):
            at = int(self.off[k]) + self.erased[k] * self.L[k]
            self.want[int(self.out_off[k]):int(self.out_off[k + 1])] = self.store[at:at + self.L[k]]
            self.store[at:at + self.L[k]] = 0
        self.out = np.zeros_like(self.want)  # every arm rebuilds into here
        ob = self.out.ctypes.data
        # pointer tables, made before any clock starts
        null = U8P()
        self.flags = np.zeros((n, t), np.uint8)
        slots = []
        for k in range(n):
            at, L = int(self.off[k]), self.L[k]
            row = [null] * t
            for i in self.loaded[k]:
                row[i] = ctypes.cast(sb + at + i * L, U8P)
                self.flags[k, i] = 1
            row[self.erased[k]] = ctypes.cast(ob + int(self.out_off[k]), U8P)
            slots.append(row)
        self.all_ptrs = (U8P * (n * t))(*[x for row in slots for x in row])
        self.all_lens = (ctypes.c_size_t * n)(*self.L)
        self.part_ptrs = [(U8P * t)(*row) for row in slots]
        self.part_lens = [(ctypes.c_size_t * t)(*([L] * t)) for L in self.L]
        self.hash_ptrs = [(U8P * d)(*[slots[k][i] for i in self.loaded[k]]) for k in range(n)]
        self.hash_lens = [(ctypes.c_size_t * d)(*([L] * d)) for L in self.L]
        self.verified = np.zeros((n, t), np.uint8)
        self.status = (ctypes.c_int * n)()

    def _check_digests(self, k, dig):
        want = self.expected[k, self.loaded[k]]
        assert np.array_equal(dig.reshape(self.d, 32), want), k

    def arm_percall(self, threads, count=None):
        h, d, t = self.rs.handle, self.d, self.t

        def one(k):
            dig = np.zeros(d * 32, np.uint8)
            st = ce._lib.cec_sha256_many(self.hash_ptrs[k], self.hash_lens[k], d,
                                         dig.ctypes.data_as(U8P))
            assert st == 0, (st, k)
            self._check_digests(k, dig)
            pres = (ctypes.c_uint8 * t)(*self.flags[k])
            st = ce._lib.cec_reconstruct_data(h, self.part_ptrs[k], self.part_lens[k], pres, t)
            assert st == 0, (st, k)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(count or self.n)))

    def arm_part_read(self, threads, count=None):
        """The per-part way in one call per part: cec_part_read (coalesced)."""
        h, t = self.rs.handle, self.t
        fb, eb, vb = (x.ctypes.data for x in (self.flags, self.expected, self.verified))

        def one(k):
            st = ce._lib.cec_part_read(h, self.part_ptrs[k], self.L[k],
                                       ctypes.cast(fb + k * t, U8P),
                                       ctypes.cast(eb + k * t * 32, U8P), 1,
                                       ctypes.cast(vb + k * t, U8P))
            assert st == 0, (st, k)
        n = count or self.n
        self.verified[:n] = 0
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(n)))
        assert np.array_equal(self.verified[:n], self.flags[:n])

    def arm_ragged(self, count=None):
        n = count or self.n
        ce._check(ce._lib.cec_parts_read(
            self.rs.handle, self.all_ptrs, self.all_lens, n, self.flags.ctypes.data_as(U8P),
            self.expected.ctypes.data_as(U8P), 1, self.verified.ctypes.data_as(U8P), self.status))
        assert all(s == 0 for s in self.status[:n])
        assert np.array_equal(self.verified[:n], self.flags[:n])

    def parts_read_d2h_bytes(self):
        """What arm b's copy back moves: per round (at most CEC_COALESCE_MAX_MIB of padded data
        chunks, ragged.cpp run_rounds) the rebuilt chunks' spans in the round's layout, neighbours
        sharing a copy while the gap between them is under 256 KiB (copy_spans)."""
        cap = int(os.environ.get("CEC_COALESCE_MAX_MIB", "1024")) << 20
        d, t, gap = self.d, self.t, 256 << 10
        total = copies = 0
        off = acc = 0
        last_to = None
        for k, L in enumerate(self.L):
            cs = (L + 15) // 16 * 16
            b = d * cs
            if acc and (b > cap or acc > cap - b):  # a new round: its own arena offsets
                off, acc, last_to = 0, 0, None
            acc += min(b, cap)
            lo = off + self.erased[k] * cs
            if last_to is not None and lo - last_to < gap:
                total += lo + L - last_to
            else:
                total += L
                copies += 1
            last_to = lo + L
            off += t * cs
        return total, copies

    def make_reader(self, slot_bytes, depth, max_parts=4096):
        """(reader, [(k0, k1)], per batch (slot pointers, chunk lengths)): consecutive parts whose
        ragged layout fits a slot, the tables made before any clock starts."""
        t = self.t
        need = [t * ((L + 15) // 16 * 16) for L in self.L]
        slot_bytes = max(slot_bytes, max(need))
        batches, k0, acc = [], 0, 0
        for k, b in enumerate(need):
            if k > k0 and (acc + b > slot_bytes or k - k0 >= max_parts):
                batches.append((k0, k))
                k0, acc = k, 0
            acc += b
        batches.append((k0, self.n))
        rd = ce.PartsReader(self.rs, slot_bytes, max_parts, depth, True)
        tables = [((U8P * ((k1 - k0) * t))(*self.all_ptrs[k0 * t:k1 * t]),
                   (ctypes.c_size_t * (k1 - k0))(*self.L[k0:k1])) for k0, k1 in batches]
        return rd, batches, tables

    def arm_reader(self, reader):
        rd, batches, tables = reader
        lib, t = ce._lib, self.t
        fb, eb = self.flags.ctypes.data, self.expected.ctypes.data
        pending = []

        def collect():
            slot, (k0, k1), ptrs = pending.pop(0)
            ver, st, n = U8P(), ctypes.POINTER(ctypes.c_int)(), ctypes.c_size_t(0)
            ce._check(lib.cec_parts_reader_wait(rd._h, slot, ctypes.byref(ver), ctypes.byref(st),
                                                None, None, ctypes.byref(n)))
            ce._check(lib.cec_parts_reader_scatter(rd._h, slot, ptrs))
            m = k1 - k0
            assert n.value == m
            assert not np.ctypeslib.as_array(st, shape=(m,)).any()
            assert np.array_equal(np.ctypeslib.as_array(ver, shape=(m, t)), self.flags[k0:k1])
        for (k0, k1), (ptrs, lens) in zip(batches, tables):
            if len(pending) == rd.depth:
                collect()
            slot, _ = rd.acquire()
            ce._check(lib.cec_parts_reader_submit_from(
                rd._h, slot, ptrs, lens, k1 - k0, ctypes.cast(fb + k0 * t, U8P),
                ctypes.cast(eb + k0 * t * 32, U8P)))
            pending.append((slot, (k0, k1), ptrs))
        while pending:
            collect()

    def arm_cpu(self, threads=16, count=None):
        lib = oracle.lib()
        d, p, t = self.d, self.p, self.t

        def one(k):
            dig = np.zeros(d * 32, np.uint8)
            for j in range(d):
                lib.or_sha256(self.hash_ptrs[k][j], self.L[k],
                              ctypes.cast(dig.ctypes.data + 32 * j, U8P))
            self._check_digests(k, dig)
            pres = (ctypes.c_uint8 * t)(*self.flags[k])
            lens = (ctypes.c_size_t * t)(*[self.L[k] if f else 0 for f in self.flags[k]])
            st = lib.or_rs_reconstruct(d, p, self.part_ptrs[k], lens, pres, t, 1)
            assert st == 0, (st, k)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(count or self.n)))


def host_read(args):
    pool, files = make_files(args.files)
    results = []
    for shape in args.shapes.split(":"):
        d, p = (int(x) for x in shape.split(","))
        w = ReadWorkload(pool, files, d, p)
        print(f"== read RS({d},{p}) chunk 1 MiB: {len(files)} files, "
              f"{w.file_bytes / 2**30:.2f} GiB, {w.n} parts, one data chunk of each erased",
              flush=True)
        arms = [("a: sha256_many + reconstruct_data x 10 threads", lambda c=None: w.arm_percall(10, c)),
                ("a: sha256_many + reconstruct_data x 256 threads",
                 lambda c=None: w.arm_percall(256, c)),
                ("a: part_read x 10 threads", lambda c=None: w.arm_part_read(10, c)),
                ("a: part_read x 256 threads", lambda c=None: w.arm_part_read(256, c)),
                ("b: one parts_read call", lambda c=None: w.arm_ragged(c)),
                ("c: CPU oracle x 16 threads", lambda c=None: w.arm_cpu(16, c))]
        if args.no_per_part:  # a quick look at b and d: the per-part arms take most of a run
            arms = [arm for arm in arms if not arm[0].startswith("a")]
        if args.per_part_only:  # the per-part arms alone
            arms = [arm for arm in arms if arm[0].startswith("a")]
            args.depths = []
        readers = {depth: w.make_reader(args.slot_mib << 20, depth) for depth in args.depths}
        d_names = {depth: f"d: parts reader (submit_from) {args.slot_mib} MiB x {depth}"
                   for depth in readers}
        for depth, reader in readers.items():
            arms.append((d_names[depth], lambda c=None, reader=reader: w.arm_reader(reader)))
        warm = min(w.n, 512)
        for name, fn in arms:  # warm-up: b and d on the whole input (b's staging is sized by it)
            sec, _ = timed(lambda: fn(None if name[0] in "bd" else warm))
            print(f"   warm-up {name}: {sec:.3f} s", flush=True)
        if readers:
            print(f"   d: {len(readers[args.depths[0]][1])} batches", flush=True)
        secs = {name: [] for name, _ in arms}
        down = {name: [] for name in d_names.values()}
        by_name = {name: readers[depth][0] for depth, name in d_names.items()}
        for rep in range(args.repeats):
            for name, fn in arms:
                w.out[:] = 0
                before = by_name[name].stats() if name in by_name else None
                sec, _ = timed(fn)
                secs[name].append(sec)
                assert np.array_equal(w.out, w.want), f"rebuilt chunks of '{name}' differ"
                note = ""
                if before is not None:
                    after = by_name[name].stats()
                    down[name].append(after[1] - before[1])
                    note = f"  D2H {down[name][-1]} B, tail copies {after[2] - before[2]}"
                print(f"   repeat {rep + 1} {name}: {sec:.3f} s  "
                      f"{w.file_bytes / sec / 1e9:7.2f} GB/s  {w.n / sec:9.0f} parts/s{note}",
                      flush=True)
        print("   every arm rebuilt the erased chunks exactly, in every repeat")
        row = {"d": d, "p": p, "files": len(files), "parts": w.n,
               "file_bytes": w.file_bytes, "seconds": secs,
               "gbps": {k: [w.file_bytes / s / 1e9 for s in v] for k, v in secs.items()}}
        if not args.no_per_part:
            for th in (10, 256):
                two = secs[f"a: sha256_many + reconstruct_data x {th} threads"]
                one = secs[f"a: part_read x {th} threads"]
                print(f"   per part, {th} threads: two calls {min(two):.3f}-{max(two):.3f} s, "
                      f"part_read {min(one):.3f}-{max(one):.3f} s "
                      f"({w.file_bytes / max(one) / 1e9:.2f}-{w.file_bytes / min(one) / 1e9:.2f} "
                      f"GB/s)", flush=True)
        if args.per_part_only:
            results.append(row)
            del w, readers, by_name
            continue
        b = secs["b: one parts_read call"]
        if not args.no_per_part:
            names = [name for name, _ in arms if name.startswith("a")]
            wins = [b[r] < min(secs[name][r] for name in names) for r in range(args.repeats)]
            print(f"   b faster than the best per-part arm in each repeat: {wins}", flush=True)
            row["b_faster_each_repeat"] = wins
        b_down, b_copies = w.parts_read_d2h_bytes()
        rebuilt = int(sum(w.L))
        print(f"   D2H per pass: rebuilt chunks {rebuilt} B; b's copy_spans {b_down} B in "
              f"{b_copies} copies ({b_down / rebuilt:.2f}x); d {sorted(set(sum(down.values(), [])))} B",
              flush=True)
        row["d2h_bytes"] = {"rebuilt": rebuilt, "b": b_down, "b_copies": b_copies, "d": down}
        for depth, name in d_names.items():
            dd = secs[name]
            spread = max(max(dd) - min(dd), max(b) - min(b))
            wins = max(dd) + spread < min(b)
            row[f"d{depth}_vs_b"] = {"b_best_s": min(b), "d_worst_s": max(dd), "spread_s": spread,
                                     "d_wins_by_more_than_spread": wins}
            print(f"   d (depth {depth}) vs b: b {min(b):.3f}-{max(b):.3f} s "
                  f"({w.file_bytes / max(b) / 1e9:.2f}-{w.file_bytes / min(b) / 1e9:.2f} GB/s), "
                  f"d {min(dd):.3f}-{max(dd):.3f} s "
                  f"({w.file_bytes / max(dd) / 1e9:.2f}-{w.file_bytes / min(dd) / 1e9:.2f} GB/s), "
                  f"largest spread {spread:.3f} s -> d wins by more than the spread: {wins}",
                  flush=True)
        results.append(row)
        del w, readers, by_name
    print(json.dumps({"tool": "small_files_bench", "mode": "host-read", "results": results}))


class VerifyWorkload:
    """The parts of `files` as the oracle stores them (d data + p parity chunks of L_k bytes,
    digests); every chunk is one copy to verify.  The first byte of the last chunk of part n // 2
    is flipped, so every arm has one bad copy to find."""

    def __init__(self, pool, files, d, p):
        self.d, self.p, self.t = d, p, d + p
        self.parts = cut_parts(files, d)
        self.n = n = len(self.parts)
        self.file_bytes = sum(s for _, s in files)
        self.L = [(ln + d - 1) // d for _, ln in self.parts]
        t = self.t
        self.off, self.store, self.expected = oracle_store(pool, self.parts, self.L, d, p)
        sb = self.store.ctypes.data
        self.stored_bytes = int(self.off[-1])
        self.want = np.ones((n, t), np.uint8)
        bad = n // 2
        self.store[int(self.off[bad]) + (t - 1) * self.L[bad]] ^= 0x01
        self.want[bad, t - 1] = 0
        # pointer tables, made before any clock starts
        self.part_ptrs = [(U8P * t)(*[ctypes.cast(sb + int(self.off[k]) + i * self.L[k], U8P)
                                      for i in range(t)]) for k in range(n)]
        self.part_lens = [(ctypes.c_size_t * t)(*([L] * t)) for L in self.L]
        self.all_ptrs = (U8P * (n * t))(*[x for row in self.part_ptrs for x in row])
        self.all_lens = (ctypes.c_size_t * (n * t))(*[L for L in self.L for _ in range(t)])
        self.ok = np.zeros((n, t), np.uint8)  # every arm's flags land here

    def arm_percall(self, threads, count=None):
        t = self.t

        def one(k):
            dig = np.zeros((t, 32), np.uint8)
            st = ce._lib.cec_sha256_many(self.part_ptrs[k], self.part_lens[k], t,
                                         dig.ctypes.data_as(U8P))
            assert st == 0, (st, k)
            self.ok[k] = (dig == self.expected[k]).all(axis=1)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(count or self.n)))

    def arm_ragged(self, count=None):
        n = count or self.n
        ce._check(ce._lib.cec_parts_verify(self.all_ptrs, self.all_lens, n * self.t,
                                           self.expected.ctypes.data_as(U8P),
                                           self.ok.ctypes.data_as(U8P)))

    def damage_more(self, every=97):
        """One byte flipped in every `every`-th copy beyond the constructor's one: its first, a
        middle or its last byte in turn."""
        t = self.t
        for x in range(0, self.n * t, every):
            k, i = divmod(x, t)
            if not self.want[k, i]:
                continue
            L = self.L[k]
            self.store[int(self.off[k]) + i * L + (0, L // 2, L - 1)[(x // every) % 3]] ^= 0x20
            self.want[k, i] = 0

    def make_scrub_pipeline(self, slot_bytes, depth, segment, max_entries=4096, max_open=None):
        """A cec_scrub_pipeline and the plan of its batches, made before any clock starts: each
        batch takes the next segment of every open copy, in copy order, then new copies while the
        slot, max_entries and the open ids last (the rule of FileReference::verify_many_stream).
        Per batch: the call's arrays (the expected rows of the entries that end a copy among
        them) and, for those entries, their rows and copies."""
        t, n = self.t, self.n * self.t
        lens = [L for L in self.L for _ in range(t)]
        slot_bytes = max(slot_bytes, ce.ragged_stride(min(segment, max(lens))))
        if not max_open:  # as many open copies as a slot holds segments (the C++ default)
            max_open = max(1, slot_bytes // ce.ragged_stride(segment))
        pl = ce.ScrubPipeline(slot_bytes, max_entries, depth, max_open)
        exp = self.expected.reshape(n, 32)
        free, open_copies, nxt, plan, most_open = list(range(max_open))[::-1], [], 0, [], 0
        while nxt < n or open_copies:
            batch, room, still, freed = [], slot_bytes, [], []

            def fits(ln):
                return len(batch) < max_entries and ce.ragged_stride(ln) <= room
            for x, done, oid in open_copies:
                ln = min(segment, lens[x] - done)
                if not fits(ln):
                    still.append((x, done, oid))
                    continue
                batch.append((x, done, ln, oid))
                room -= ce.ragged_stride(ln)
                if done + ln == lens[x]:
                    freed.append(oid)
                else:
                    still.append((x, done + ln, oid))
            while nxt < n:
                ln = min(segment, lens[nxt])
                whole = ln == lens[nxt]
                if not fits(ln) or (not whole and not free):
                    break
                oid = 0 if whole else free.pop()
                if not whole:
                    still.append((nxt, ln, oid))
                batch.append((nxt, 0, ln, oid))
                room -= ce.ragged_stride(ln)
                nxt += 1
            free += freed
            open_copies = still
            most_open = max(most_open, len(still))
            m = len(batch)
            last = [q for q, (x, off, ln, _) in enumerate(batch) if off + ln == lens[x]]
            rows = np.zeros((m, 32), np.uint8)
            rows[last] = exp[[batch[q][0] for q in last]]
            plan.append({
                "m": m,
                "bufs": (U8P * m)(*[self.all_ptrs[x] for x, _, _, _ in batch]),
                "lens": (ctypes.c_size_t * m)(*[lens[x] for x, _, _, _ in batch]),
                "offs": (ctypes.c_size_t * m)(*[e[1] for e in batch]),
                "segs": (ctypes.c_size_t * m)(*[e[2] for e in batch]),
                "ids": (ctypes.c_uint32 * m)(*[e[3] for e in batch]),
                "rows": rows,
                "last_rows": np.array(last, np.int64),
                "last_copies": np.array([batch[q][0] for q in last], np.int64)})
        return pl, plan, most_open

    def arm_scrub(self, pipe):
        """Every planned batch through the scrub pipeline's slots; while later slots run the
        oldest is collected: the flags of the entries that end a copy copied into self.ok."""
        pl, plan, _ = pipe
        lib, h = ce._lib, pl._h
        flat = self.ok.reshape(-1)
        slot, okp, n = ctypes.c_size_t(0), U8P(), ctypes.c_size_t(0)
        pending = []

        def collect():
            s, b = pending.pop(0)
            ce._check(lib.cec_scrub_pipeline_wait(h, s, ctypes.byref(okp), ctypes.byref(n)))
            assert n.value == b["m"]
            flat[b["last_copies"]] = np.ctypeslib.as_array(okp, shape=(b["m"],))[b["last_rows"]]
        for b in plan:
            if len(pending) == pl.depth:
                collect()
            ce._check(lib.cec_scrub_pipeline_acquire(h, ctypes.byref(slot)))
            ce._check(lib.cec_scrub_pipeline_submit_from(
                h, slot.value, b["bufs"], b["lens"], b["offs"], b["segs"], b["ids"],
                b["rows"].ctypes.data_as(U8P), b["m"]))
            pending.append((slot.value, b))
        while pending:
            collect()
        assert pl.open_count() == 0

    def arm_cpu(self, threads=16, count=None):
        lib = oracle.lib()
        t = self.t

        def one(k):
            dig = np.zeros((t, 32), np.uint8)
            for i in range(t):
                lib.or_sha256(self.part_ptrs[k][i], self.L[k],
                              ctypes.cast(dig.ctypes.data + 32 * i, U8P))
            self.ok[k] = (dig == self.expected[k]).all(axis=1)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(count or self.n)))


def host_verify(args):
    pool, files = make_files(args.files)
    results = []
    for shape in args.shapes.split(":"):
        d, p = (int(x) for x in shape.split(","))
        w = VerifyWorkload(pool, files, d, p)
        print(f"== verify RS({d},{p}) chunk 1 MiB: {len(files)} files, "
              f"{w.file_bytes / 2**30:.2f} GiB in {w.stored_bytes / 2**30:.2f} GiB of chunks, "
              f"{w.n} parts, {w.n * w.t} copies, one of them flipped", flush=True)
        arms = [("a: sha256_many per part x 10 threads", lambda c=None: w.arm_percall(10, c)),
                ("a: sha256_many per part x 256 threads", lambda c=None: w.arm_percall(256, c)),
                ("b: one parts_verify call", lambda c=None: w.arm_ragged(c)),
                ("c: CPU oracle x 16 threads", lambda c=None: w.arm_cpu(16, c))]
        warm = min(w.n, 512)
        for name, fn in arms:  # warm-up: b on the whole input (its staging is sized by it)
            sec, _ = timed(lambda: fn(None if name.startswith("b") else warm))
            print(f"   warm-up {name}: {sec:.3f} s", flush=True)
        secs = {name: [] for name, _ in arms}
        for rep in range(args.repeats):
            for name, fn in arms:
                w.ok[:] = 7
                sec, _ = timed(fn)
                secs[name].append(sec)
                assert np.array_equal(w.ok, w.want), f"flags of '{name}' differ"
                print(f"   repeat {rep + 1} {name}: {sec:.3f} s  "
                      f"{w.stored_bytes / sec / 1e9:7.2f} GB/s of chunks  "
                      f"{w.file_bytes / sec / 1e9:7.2f} GB/s of files  {w.n / sec:9.0f} parts/s",
                      flush=True)
        print("   every arm found every copy good and the flipped one bad, in every repeat")
        names = [name for name, _ in arms]
        wins = [secs[names[2]][r] < min(secs[names[0]][r], secs[names[1]][r])
                for r in range(args.repeats)]
        print(f"   b faster than the better per-part arm in each repeat: {wins}", flush=True)
        results.append({"d": d, "p": p, "files": len(files), "parts": w.n,
                        "file_bytes": w.file_bytes, "stored_bytes": w.stored_bytes,
                        "seconds": secs,
                        "gbps_stored": {k: [w.stored_bytes / s / 1e9 for s in v]
                                        for k, v in secs.items()},
                        "b_faster_each_repeat": wins})
        del w
    print(json.dumps({"tool": "small_files_bench", "mode": "host-verify", "results": results}))


def host_verify_segments(args):
    """--verify --segment: the one parts_verify call (arm a) and the scrub pipeline at these
    segment sizes (arm c) over the same copies, some of them damaged, alternating."""
    pool, files = make_files(args.files)
    results = []
    slot = args.slot_mib << 20
    for shape in args.shapes.split(":"):
        d, p = (int(x) for x in shape.split(","))
        w = VerifyWorkload(pool, files, d, p)
        w.damage_more()
        print(f"== scrub RS({d},{p}) chunk 1 MiB: {len(files)} files, "
              f"{w.stored_bytes / 2**30:.2f} GiB of chunks, {w.n} parts, {w.n * w.t} copies, "
              f"{int((w.want == 0).sum())} of them damaged, longest copy {max(w.L)} bytes",
              flush=True)
        arms = [("a: one parts_verify call", w.arm_ragged)]
        info = {}
        for seg in args.segment:
            for depth in args.depths:
                size = f"{seg >> 10} KiB" if seg % 1024 == 0 else f"{seg} B"
                name = f"c: scrub pipeline {size} segments, {args.slot_mib} MiB x {depth}"
                pipe = w.make_scrub_pipeline(slot, depth, seg, max_open=args.max_open)
                arms.append((name, lambda pipe=pipe: w.arm_scrub(pipe)))
                info[name] = {"batches": len(pipe[1]), "max_open": pipe[0].max_open,
                              "most_open": pipe[2]}
                print(f"   {name}: {len(pipe[1])} batches, up to {pipe[2]} copies open "
                      f"(of {pipe[0].max_open} ids)", flush=True)
        for name, fn in arms:
            w.ok[:] = 7
            sec, _ = timed(fn)
            assert np.array_equal(w.ok, w.want), f"flags of '{name}' differ (warm-up)"
            print(f"   warm-up {name}: {sec:.3f} s", flush=True)
        secs = {name: [] for name, _ in arms}
        for rep in range(args.repeats):
            for name, fn in arms:
                w.ok[:] = 7
                sec, _ = timed(fn)
                secs[name].append(sec)
                assert np.array_equal(w.ok, w.want), f"flags of '{name}' differ"
                print(f"   repeat {rep + 1} {name}: {sec:.3f} s  "
                      f"{w.stored_bytes / sec / 1e9:7.2f} GB/s of copies", flush=True)
        print("   every arm's flags equal arm a's (and the damage done), in every repeat")
        gbps = {k: [w.stored_bytes / x / 1e9 for x in v] for k, v in secs.items()}
        row = {"d": d, "p": p, "files": len(files), "parts": w.n, "copies": w.n * w.t,
               "stored_bytes": w.stored_bytes, "seconds": secs, "gbps_stored": gbps,
               "pipelines": info, "verdicts": {}}
        inc = arms[0][0]
        for name in info:
            wins = min(gbps[name]) > max(gbps[inc])
            row["verdicts"][f"{name} over {inc}"] = wins
            print(f"   {name}: {min(gbps[name]):.2f}-{max(gbps[name]):.2f} GB/s against {inc}: "
                  f"{min(gbps[inc]):.2f}-{max(gbps[inc]):.2f} GB/s -> worst above the "
                  f"incumbent's best: {wins}", flush=True)
        results.append(row)
        del w, arms
    print(json.dumps({"tool": "small_files_bench", "mode": "verify-segment", "results": results}))


def device_read(args):
    d, p, n, L = 10, 4, 4096, 65536
    t = d + p
    dev = torch.device("cuda", 0)
    rs = ce.ReedSolomon(d, p)
    full = torch.zeros((n, t, L), dtype=torch.uint8, device=dev)
    batch_full = ce.PartBatch.from_tensor(full, L)
    ce.fill_synthetic(batch_full, d, 1)
    ce.encode_batch(rs, batch_full)
    present = np.ones((n, t), np.uint8)
    for k in range(n):  # two erasures per part: one data chunk, one other chunk
        present[k, [k % d, (k + 3) % t if (k + 3) % t != k % d else (k + 4) % t]] = 0
    gone = torch.from_numpy(present == 0).to(dev)
    pres = present.tobytes()
    buf = full.clone()
    batch = ce.PartBatch.from_tensor(buf, L)
    offs, total = ce.ragged_layout(t, [L] * n)
    assert total == buf.numel()
    lens = [L] * n

    def uniform():
        ce.reconstruct_batch(rs, batch, pres, False)

    def ragged():
        ce.reconstruct_ragged(rs, buf.data_ptr(), offs, lens, pres, False)

    def run(fn):
        buf[gone] = 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        assert torch.equal(buf, full), "rebuilt chunks differ"
        return e0.elapsed_time(e1)

    for fn in (uniform, ragged):
        run(fn)
    ms = {"reconstruct_batch": [], "reconstruct_ragged": []}
    for rep in range(args.repeats):
        ms["reconstruct_batch"].append(run(uniform))
        ms["reconstruct_ragged"].append(run(ragged))
    print(f"== device resident read, {n} x RS({d},{p}) x {L} B, two erasures per part")
    for k, v in ms.items():
        print(f"   {k}: " + "  ".join(f"{x:.3f} ms" for x in v))
    ratio = min(ms["reconstruct_ragged"]) / min(ms["reconstruct_batch"])
    print(f"   ragged / uniform (best of {args.repeats}): {ratio:.3f}   (same rebuilt chunks)")
    print(json.dumps({"tool": "small_files_bench", "mode": "device-read", "ms": ms,
                      "ratio": ratio}))


def _ranges(ms):
    return {k: [min(v), max(v)] for k, v in ms.items()}


def read_async_arms(args, name, rs, buf, start, want, offs, lens, flags, dexp):
    """cec_read_ragged against cec_read_ragged_async on one device-resident batch (`start`: the
    buffer with the erased chunks zeroed, `want`: what a read must leave).  (a) one call over
    all parts: the interval between two stream events around it and the host's wall time inside
    the call.  (b) the parts cut into two halves on two streams from one thread: wall time from
    before the first call to after the second stream's synchronise.  Arms alternate after a
    warm-up; every run's buffer, flags and statuses are compared with `want` and between arms."""
    n, t = len(lens), rs.total_shard_count()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    h = n // 2
    halves = [(0, h), (h, n)]
    ver = ce.HostBuffer(n * t)
    st = ce.HostBuffer(n * 4)

    def call(use_async, lo, hi, stream):
        pres = flags[lo:hi].tobytes()
        exp = dexp.data_ptr() + lo * t * 32
        if use_async:
            ce.read_ragged_async(rs, buf.data_ptr(), offs[lo:hi], lens[lo:hi], pres, exp,
                                 ver.array[lo * t:hi * t], st.array[lo * 4:hi * 4], stream)
        else:
            v, s = ce.read_ragged(rs, buf.data_ptr(), offs[lo:hi], lens[lo:hi], pres, exp, stream)
            ver.array[lo * t:hi * t] = np.frombuffer(v, np.uint8)
            st.array[lo * 4:hi * 4] = np.array(s, np.int32).view(np.uint8)

    answers = {}

    def settle(use_async):
        """After a run: the buffer against `want`, the outputs against the other arm's."""
        assert torch.equal(buf, want), f"{name}: rebuilt bytes differ (async={use_async})"
        out = (ver.array.tobytes(), st.array.tobytes())
        assert answers.setdefault("out", out) == out, f"{name}: flags or statuses differ"
        assert (st.array.view(np.int32) == ce.OK).all()

    def reset():
        buf.copy_(start)
        ver.array[:] = 0xEE
        st.array[:] = 0xEE
        torch.cuda.synchronize()

    def single(use_async):
        reset()
        s = streams[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        t0 = time.perf_counter()
        call(use_async, 0, n, s)
        t1 = time.perf_counter()
        e1.record(s)
        s.synchronize()
        settle(use_async)
        return e0.elapsed_time(e1), (t1 - t0) * 1e3

    def pair(use_async):
        reset()
        t0 = time.perf_counter()
        for (lo, hi), s in zip(halves, streams):
            call(use_async, lo, hi, s)
        for s in streams:
            s.synchronize()
        t1 = time.perf_counter()
        settle(use_async)
        return (t1 - t0) * 1e3

    for use_async in (False, True):  # warm-up: code objects, scratch buffers, the codec's copies
        single(use_async)
        pair(use_async)
    ms = {k: [] for k in ("sync_event", "async_event", "sync_call", "async_call", "sync_pair",
                          "async_pair")}
    for rep in range(args.repeats):
        for use_async, arm in ((False, "sync"), (True, "async")):
            ev, wall = single(use_async)
            ms[arm + "_event"].append(ev)
            ms[arm + "_call"].append(wall)
        for use_async, arm in ((False, "sync"), (True, "async")):
            ms[arm + "_pair"].append(pair(use_async))
    spread = max(max(v) - min(v) for v in ms.values())
    gain = max(ms["async_pair"]) < min(ms["sync_pair"])
    r = _ranges(ms)
    print(f"== read, sync against async: {name}, {n} parts, chunk lengths {min(lens)}-{max(lens)} B")
    for k in ms:
        print(f"   {k}: " + "  ".join(f"{x:.3f}" for x in ms[k]) +
              f" ms   range {r[k][0]:.3f}-{r[k][1]:.3f}")
    print(f"   (a) one call: event interval async / sync (best) "
          f"{min(ms['async_event']) / min(ms['sync_event']):.3f}; host time inside the call "
          f"sync {r['sync_call'][0]:.3f}-{r['sync_call'][1]:.3f} ms, "
          f"async {r['async_call'][0]:.3f}-{r['async_call'][1]:.3f} ms")
    print(f"   (b) two halves, two streams, one thread: sync {r['sync_pair'][0]:.3f}-"
          f"{r['sync_pair'][1]:.3f} ms, async {r['async_pair'][0]:.3f}-{r['async_pair'][1]:.3f} ms; "
          f"largest spread within an arm {spread:.3f} ms -> async's worst below sync's best: {gain}",
          flush=True)
    return {"ms": ms, "spread_ms": spread, "async_pair_gain": gain}


def device_read_async(args):
    """The arms of read_async_arms on --device --read's batch and on the tool's own files as
    device-resident RS(10,4) and RS(3,2) parts with data chunk k % d of part k erased."""
    dev = torch.device("cuda", 0)
    results = {}
    # --device --read's batch
    d, p, n, L = 10, 4, 4096, 65536
    t = d + p
    rs = ce.ReedSolomon(d, p)
    full = torch.zeros((n, t, L), dtype=torch.uint8, device=dev)
    dexp = torch.zeros((n, t, 32), dtype=torch.uint8, device=dev)
    batch = ce.PartBatch.from_tensor(full, L)
    ce.fill_synthetic(batch, d, 1)
    ce.encode_hash_batch(rs, batch, dexp.data_ptr())
    flags = np.ones((n, t), np.uint8)
    for k in range(n):
        flags[k, [k % d, (k + 3) % t if (k + 3) % t != k % d else (k + 4) % t]] = 0
    gone = torch.from_numpy(flags == 0).to(dev)
    start = full.clone()
    start[gone] = 0
    want = start.clone()  # a read rebuilds the data chunks and leaves missing parity alone
    want[:, :d] = full[:, :d]
    offs, total = ce.ragged_layout(t, [L] * n)
    buf = start.clone()
    results["uniform_10_4_64k"] = read_async_arms(
        args, f"{n} x RS({d},{p}) x {L} B, two erasures per part", rs, buf.view(-1),
        start.view(-1), want.view(-1), offs, [L] * n, flags, dexp)
    del full, start, want, buf, gone, dexp
    pool, files = make_files(args.files)
    for d, p in ((10, 4), (3, 2)):
        t = d + p
        rs = ce.ReedSolomon(d, p)
        parts = cut_parts(files, d)
        n = len(parts)
        lens = [(ln + d - 1) // d for _, ln in parts]
        offs, total = ce.ragged_layout(t, lens)
        host = np.zeros(total, np.uint8)
        for (o, ln), off, L in zip(parts, offs, lens):
            cs = ce.ragged_stride(L)
            for j in range(d):
                have = max(0, min(L, ln - j * L))
                host[off + j * cs:off + j * cs + have] = pool[o + j * L:o + j * L + have]
        want = torch.from_numpy(host).to(dev)
        del host
        dexp = torch.zeros((n, t, 32), dtype=torch.uint8, device=dev)
        ce.encode_hash_ragged(rs, want.data_ptr(), offs, lens, dexp.data_ptr())
        torch.cuda.synchronize()
        flags = np.ones((n, t), np.uint8)
        start = want.clone()
        for k, (off, L) in enumerate(zip(offs, lens)):
            flags[k, k % d] = 0
            at = off + (k % d) * ce.ragged_stride(L)
            start[at:at + L] = 0
        buf = start.clone()
        results[f"mixed_{d}_{p}"] = read_async_arms(
            args, f"{len(files)} files as RS({d},{p}) parts, one data chunk per part erased", rs,
            buf, start, want, offs, lens, flags, dexp)
        del want, start, buf, dexp
    print(json.dumps({"tool": "small_files_bench", "mode": "device-read-async",
                      "results": {k: {"ranges_ms": _ranges(v["ms"]), "spread_ms": v["spread_ms"],
                                      "async_pair_gain": v["async_pair_gain"]}
                                  for k, v in results.items()},
                      "read_stats": ce.ragged_read_stats()}))


KNOB = "CEC_RAGGED_FUSED"


def set_knob(value):
    """CEC_RAGGED_FUSED = value (None: unset) from the next call on."""
    set_env_knob(KNOB, value)


def event_ms(fn, knob=None):
    """One call of fn between two stream events, the knob set before the first."""
    set_knob(knob)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    set_knob(None)
    return e0.elapsed_time(e1)


def fused_verdict(name, two_pass, fused):
    """The rule of the pipeline's arm d, without a margin fixed in advance: fused wins a
    configuration when its worst repeat is below two-pass's best."""
    wins = max(fused) < min(two_pass)
    print(f"   {name}: two-pass {min(two_pass):.3f}-{max(two_pass):.3f} ms, fused "
          f"{min(fused):.3f}-{max(fused):.3f} ms, two-pass best / fused worst "
          f"{min(two_pass) / max(fused):.3f} -> fused's worst below two-pass's best: {wins}",
          flush=True)
    return {"two_pass_ms": two_pass, "fused_ms": fused, "fused_wins": wins}


def device_uniform(args):
    d, p, n, L = 10, 4, 4096, 65536
    t = d + p
    dev = torch.device("cuda", 0)
    rs = ce.ReedSolomon(d, p)
    buf = torch.zeros((n, t, L), dtype=torch.uint8, device=dev)
    batch = ce.PartBatch.from_tensor(buf, L)
    ce.fill_synthetic(batch, d, 1)
    dig_u = torch.zeros((n, t, 32), dtype=torch.uint8, device=dev)
    dig_r = torch.zeros_like(dig_u)
    offs, total = ce.ragged_layout(t, [L] * n)
    assert total == buf.numel()
    lens = [L] * n

    def uniform():
        ce.encode_hash_batch(rs, batch, dig_u.data_ptr())

    def ragged():
        ce.encode_hash_ragged(rs, buf.data_ptr(), offs, lens, dig_r.data_ptr())

    # the same data chunks in a region of their own, the parity in another
    sdata = buf[:, :d].contiguous()
    spar = torch.zeros((n, p, L), dtype=torch.uint8, device=dev)
    dig_s = torch.zeros_like(dig_u)
    doffs, poffs, db, pb = ce.split_layout(d, p, lens)
    assert db == sdata.numel() and pb == spar.numel()

    def split():
        ce.encode_hash_split(rs, sdata.data_ptr(), doffs, spar.data_ptr(), poffs, lens,
                             dig_s.data_ptr())

    # (name, call, CEC_RAGGED_FUSED): the ragged call by both of its paths, the split call by
    # the default
    arms = [("encode_hash_batch", uniform, None), ("encode_hash_ragged", ragged, "0"),
            ("encode_hash_ragged fused", ragged, "1"), ("encode_hash_split", split, None)]
    for _, fn, knob in arms:
        event_ms(fn, knob)
    uniform()
    torch.cuda.synchronize()
    parity = buf[:, d:].clone()
    for knob in ("0", "1"):  # each path's parity and digests against the uniform call's
        buf[:, d:] = 0
        dig_r.zero_()
        before = ce.ragged_stats()
        event_ms(ragged, knob)
        after = ce.ragged_stats()
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if knob == "1" else (0, 1))
        assert torch.equal(parity, buf[:, d:]) and torch.equal(dig_u, dig_r), "results differ"
    split()
    torch.cuda.synchronize()
    assert torch.equal(parity, spar) and torch.equal(dig_u, dig_s), "split results differ"
    ms = {name: [] for name, _, _ in arms}
    for rep in range(args.repeats):
        for name, fn, knob in arms:
            ms[name].append(event_ms(fn, knob))
    print(f"== device resident, {n} x RS({d},{p}) x {L} B ({n * d * L / 2**30:.2f} GiB of data)")
    for k, v in ms.items():
        print(f"   {k}: " + "  ".join(f"{x:.3f} ms" for x in v))
    ratio = min(ms["encode_hash_ragged"]) / min(ms["encode_hash_batch"])
    fused_ratio = min(ms["encode_hash_ragged fused"]) / min(ms["encode_hash_batch"])
    split_ratio = min(ms["encode_hash_split"]) / min(ms["encode_hash_ragged"])
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"   ragged / uniform (best of {args.repeats}): {ratio:.3f}   (same parity, same digests)")
    print(f"   fused ragged / uniform (best of {args.repeats}): {fused_ratio:.3f}")
    print(f"   split / ragged (best of {args.repeats}): {split_ratio:.3f}   largest spread between "
          f"repeats of an arm: {spread:.3f} ms")
    verdict = fused_verdict("uniform 64 KiB", ms["encode_hash_ragged"],
                            ms["encode_hash_ragged fused"])
    return {"ms": ms, "ratio": ratio, "fused_over_uniform": fused_ratio,
            "split_over_ragged": split_ratio, "spread_ms": spread}, verdict


def device_mixed(args, pool, files, d, p):
    """The tool's own files as packed device-resident parts of d x 1 MiB at most: one
    cec_encode_hash_ragged call over all of them, by the two-pass and by the fused path."""
    t = d + p
    dev = torch.device("cuda", 0)
    rs = ce.ReedSolomon(d, p)
    parts = cut_parts(files, d)
    n = len(parts)
    lens = [(ln + d - 1) // d for _, ln in parts]
    offs, total = ce.ragged_layout(t, lens)
    host = np.zeros(total, np.uint8)
    for (o, ln), off, L in zip(parts, offs, lens):  # chunk j = bytes [j*L, (j+1)*L), zeros behind
        cs = ce.ragged_stride(L)
        for j in range(d):
            have = max(0, min(L, ln - j * L))
            host[off + j * cs:off + j * cs + have] = pool[o + j * L:o + j * L + have]
    start = torch.from_numpy(host).to(dev)
    del host
    buf = start.clone()
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device=dev)

    def ragged():
        ce.encode_hash_ragged(rs, buf.data_ptr(), offs, lens, dig.data_ptr())

    results = {}
    for knob in ("0", "1"):  # warm-up, and each path's whole buffer and digests kept
        buf.copy_(start)
        dig.zero_()
        event_ms(ragged, knob)
        results[knob] = (buf.clone(), dig.clone())
    assert torch.equal(results["0"][0], results["1"][0]), "buffers differ"
    assert torch.equal(results["0"][1], results["1"][1]), "digests differ"
    assert not torch.equal(results["0"][0], start)
    del results
    ms = {"0": [], "1": []}
    for rep in range(args.repeats):
        for knob in ("0", "1"):
            ms[knob].append(event_ms(ragged, knob))
    print(f"== device resident, mixed lengths: {len(files)} files as {n} packed RS({d},{p}) parts, "
          f"chunk lengths {min(lens)}-{max(lens)} B, {sum(ln for _, ln in parts) / 2**30:.2f} GiB "
          f"of data (same buffer, same digests by both paths)")
    print("   two-pass: " + "  ".join(f"{x:.3f} ms" for x in ms["0"]))
    print("   fused:    " + "  ".join(f"{x:.3f} ms" for x in ms["1"]))
    return fused_verdict(f"mixed RS({d},{p})", ms["0"], ms["1"])


def device_mode(args):
    uniform, v1 = device_uniform(args)
    pool, files = make_files(args.files)
    verdicts = {"uniform_10_4_64k": v1}
    for d, p in ((3, 2), (10, 4)):
        verdicts[f"mixed_{d}_{p}"] = device_mixed(args, pool, files, d, p)
    fused_default = all(v["fused_wins"] for v in verdicts.values())
    print(f"== fused's worst repeat below two-pass's best in all three configurations: "
          f"{fused_default} -> the default for large ragged launches is "
          f"{'fused' if fused_default else 'two-pass'}")
    print(json.dumps({"tool": "small_files_bench", "mode": "device", **uniform,
                      "fused": verdicts, "fused_default": fused_default}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="3,2:10,4")
    ap.add_argument("--slot-mib", type=int, default=64,
                    help="arm d: data bytes per slot (--read: bytes of ragged layout per slot)")
    ap.add_argument("--depths", type=lambda s: [int(x) for x in s.split(",")], default=[3, 2],
                    help="arm d: one arm per number of slots in flight")
    ap.add_argument("--no-per-part", action="store_true",
                    help="host mode and --read: leave out the a arms")
    ap.add_argument("--per-part-only", action="store_true",
                    help="host mode and --read: the a arms alone (the CEC_COALESCE_MIXED A/B)")
    ap.add_argument("--segment", type=lambda s: [int(x) for x in s.split(",")], default=None,
                    metavar="BYTES[,BYTES...]",
                    help="the one call, the parts pipeline and the segment pipeline at these "
                         "segment sizes (multiples of 64 bytes); with --verify: the one "
                         "parts_verify call and the scrub pipeline")
    ap.add_argument("--max-open", type=int, default=0,
                    help="--segment: parts under way at most (0: as many as a slot holds segments)")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--read", action="store_true")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if args.segment and args.verify:
        host_verify_segments(args)
    elif args.segment:
        host_segments(args)
    elif args.device:
        if args.read:
            device_read(args)
            device_read_async(args)
        else:
            device_mode(args)
    elif args.verify:
        host_verify(args)
    else:
        (host_read if args.read else host_staged)(args)


if __name__ == "__main__":
    main()
