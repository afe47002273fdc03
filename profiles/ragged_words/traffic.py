"""Every ragged entry point once, RS(3,2), five parts of chunk lengths 1, 17, 4097, 65536, 683
(run under rocprofv3 HIP + kernel tracing, once with CEC_LIBRARY set to the parent's library and
once with this tree's: NOTES.md section 5)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "chunky-bits_amd"))
import numpy as np
import torch
import chunky_ec as ce

DEV = torch.device("cuda", 0)
d, p = 3, 2
t = d + p
lens = [1, 17, 4097, 65536, 683]
n = len(lens)
rs = ce.ReedSolomon(d, p)
rng = np.random.default_rng(5)
stride = [ce.ragged_stride(L) for L in lens]

offs, total = ce.ragged_layout(t, lens)
host = np.zeros(total, np.uint8)
for k, L in enumerate(lens):
    for j in range(d):
        host[offs[k] + j * stride[k]: offs[k] + j * stride[k] + L] = rng.integers(0, 256, L, dtype=np.uint8)
buf = torch.from_numpy(host).to(DEV)
dig = torch.zeros(n * t * 32, dtype=torch.uint8, device=DEV)
torch.cuda.synchronize()
print("== encode_hash_ragged", flush=True)
ce.encode_hash_ragged(rs, buf.data_ptr(), offs, lens, dig.data_ptr())
torch.cuda.synchronize()
full = buf.clone()

print("== encode_hash_split", flush=True)
doffs, poffs, db, pb = ce.split_layout(d, p, lens)
dbuf = torch.from_numpy(rng.integers(0, 256, db, dtype=np.uint8)).to(DEV)
pbuf = torch.zeros(pb, dtype=torch.uint8, device=DEV)
dig2 = torch.zeros(n * t * 32, dtype=torch.uint8, device=DEV)
torch.cuda.synchronize()
ce.encode_hash_split(rs, dbuf.data_ptr(), doffs, pbuf.data_ptr(), poffs, lens, dig2.data_ptr())
torch.cuda.synchronize()

print("== verify_ragged", flush=True)
ver = ce.verify_ragged(t, buf.data_ptr(), offs, lens, None, dig.data_ptr())
assert ver == b"\x01" * (n * t), ver

flags = np.ones((n, t), np.uint8)
for k in range(n):
    flags[k, [k % d, d + k % p]] = 0


def damaged():
    b = full.clone()
    for k in range(n):
        for i in range(t):
            if not flags[k, i]:
                b[offs[k] + i * stride[k]: offs[k] + (i + 1) * stride[k]] = 0
    torch.cuda.synchronize()
    return b


print("== read_ragged", flush=True)
b = damaged()
ver, st = ce.read_ragged(rs, b.data_ptr(), offs, lens, flags.tobytes(), dig.data_ptr())
torch.cuda.synchronize()
assert list(st) == [0] * n
for k, L in enumerate(lens):
    for i in range(d):
        a = offs[k] + i * stride[k]
        assert torch.equal(b[a:a + L], full[a:a + L]), (k, i)

print("== read_ragged_async", flush=True)
b = damaged()
hv, hs = ce.HostBuffer(n * t), ce.HostBuffer(n * 4)
ce.read_ragged_async(rs, b.data_ptr(), offs, lens, flags.tobytes(), dig.data_ptr(), hv, hs)
torch.cuda.synchronize()
assert bytes(hv.array) == flags.tobytes() and not hs.array.any()
for k, L in enumerate(lens):
    for i in range(d):
        a = offs[k] + i * stride[k]
        assert torch.equal(b[a:a + L], full[a:a + L]), (k, i)

print("== read_ragged_packed_async", flush=True)
b = damaged()
cap = sum(min(p, d) * s for s in stride)
region = torch.zeros(cap, dtype=torch.uint8, device=DEV)
ho = ce.HostBuffer((n + 1) * 8)
torch.cuda.synchronize()
ce.read_ragged_packed_async(rs, b.data_ptr(), offs, lens, flags.tobytes(), dig.data_ptr(), True,
                            hv, hs, region.data_ptr(), cap, ho)
torch.cuda.synchronize()
ro = np.frombuffer(bytes(ho.array), np.uint64)
assert ro[0] == 0 and ro[n] == sum(stride), ro  # one data chunk rebuilt per part
for k, L in enumerate(lens):
    a = offs[k] + (k % d) * stride[k]
    assert torch.equal(region[int(ro[k]):int(ro[k]) + L], full[a:a + L]), k

print("== parts_encode", flush=True)
bufs = [rng.integers(0, 256, d * L, dtype=np.uint8).tobytes() for L in lens]
enc = ce.parts_encode(rs, bufs)
assert [e.chunksize for e in enc] == lens

print("== parts_read", flush=True)
parts, expected = [], []
for k, L in enumerate(lens):
    chunks = [bufs[k][j * L:(j + 1) * L] for j in range(d)] + list(enc[k].parity)
    parts.append([c if flags[k, i] else None for i, c in enumerate(chunks)])
    expected.append([h.digest for h in enc[k].hashes])
got, ver, st = ce.parts_read(rs, parts, expected, True)
assert list(st) == [0] * n
for k, L in enumerate(lens):
    for j in range(d):
        assert bytes(got[k][j]) == bufs[k][j * L:(j + 1) * L], (k, j)
print("traffic ok", flush=True)
