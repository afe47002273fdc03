// Compute stand-ins for the host run of the scheduler and pipelines (sched_host_test.cpp): the nine
// project symbols pipeline.cpp, multi.cpp and hostmem.cpp leave undefined.  Each launch validates
// its arguments as include/chunky_ec.h and csrc/kernels.hpp document them, queues a host function
// on the given stream through the HIP stand-in, and computes with the oracle.  The arithmetic is
// not under test here; which bytes go where, in which order, under which flags, is.  As in
// csrc/capi.cpp none of them waits for the stream, and cec_reconstruct_batch reads its HOST
// present array during the call (the caller may free it on return).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "chunky_ec.h"
#include "hip_standin/standin.hpp"
#include "kernels.hpp"

extern "C" {
void or_sha256(const uint8_t* buf, size_t len, uint8_t out[32]);
int or_rs_encode_sep(size_t d, size_t p, const uint8_t* const* data, const size_t* data_lens,
                     size_t n_data, uint8_t* const* parity, const size_t* parity_lens,
                     size_t n_parity);
int or_rs_reconstruct(size_t d, size_t p, uint8_t* const* shards, const size_t* lens,
                      uint8_t* present, size_t n_shards, int data_only);
}

struct cec_codec {
    size_t d, p;
};

namespace {

thread_local std::string g_error;

int batch_ok(const cec_part_batch* b, size_t t, const char* what) {
    if (!b || !b->base) return CEC_ERR_INVALID_ARGUMENT;
    if (b->n_parts == 0) return CEC_OK;
    if (b->chunk_len == 0) return CEC_EMPTY_SHARD;
    if (b->chunk_stride < b->chunk_len || b->part_stride < t * b->chunk_stride)
        return CEC_ERR_INVALID_ARGUMENT;
    standin_check_device_range(
        b->base, (b->n_parts - 1) * b->part_stride + (t - 1) * b->chunk_stride + b->chunk_len, what);
    return CEC_OK;
}

int queued(hipError_t e, const char* what) {
    if (e == hipSuccess) return CEC_OK;
    g_error = std::string(what) + ": " + hipGetErrorString(e);
    return CEC_ERR_HIP;
}

}  // namespace

extern "C" {

const char* cec_last_error(void) { return g_error.c_str(); }

int cec_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int cec_codec_new(size_t d, size_t p, cec_codec** out) {
    if (!out) return CEC_ERR_INVALID_ARGUMENT;
    *out = new cec_codec{d, p};
    return CEC_OK;
}
void cec_codec_free(cec_codec* c) { delete c; }
size_t cec_codec_data_shards(const cec_codec* c) { return c ? c->d : 0; }
size_t cec_codec_parity_shards(const cec_codec* c) { return c ? c->p : 0; }

int cec_encode_hash_batch(const cec_codec* c, const cec_part_batch* b, uint8_t* digests,
                          void* stream) {
    if (!c || !digests) return CEC_ERR_INVALID_ARGUMENT;
    const size_t d = c->d, p = c->p, t = d + p;
    const int st = batch_ok(b, t, "cec_encode_hash_batch");
    if (st != CEC_OK || b->n_parts == 0) return st;
    standin_check_device_range(digests, b->n_parts * t * 32, "cec_encode_hash_batch digests");
    const cec_part_batch bb = *b;
    auto fn = [=] {
        std::vector<const uint8_t*> dp(d);
        std::vector<uint8_t*> pp(p);
        const std::vector<size_t> dl(d, bb.chunk_len), pl(p, bb.chunk_len);
        for (size_t k = 0; k < bb.n_parts; ++k) {
            uint8_t* part = bb.base + k * bb.part_stride;
            for (size_t j = 0; j < d; ++j) dp[j] = part + j * bb.chunk_stride;
            for (size_t i = 0; i < p; ++i) pp[i] = part + (d + i) * bb.chunk_stride;
            (void)or_rs_encode_sep(d, p, dp.data(), dl.data(), d, pp.data(), pl.data(), p);
            for (size_t i = 0; i < t; ++i)
                or_sha256(part + i * bb.chunk_stride, bb.chunk_len, digests + (k * t + i) * 32);
        }
    };
    return queued(standin_enqueue(static_cast<hipStream_t>(stream), "encode_hash", fn,
                                  {bb.base, digests}),
                  "encode_hash");
}

int cec_verify_batch(const cec_part_batch* b, size_t first_chunk, size_t n_chunks,
                     const uint8_t* present, const uint8_t* expected, uint8_t* ok, void* stream) {
    const int st = batch_ok(b, first_chunk + n_chunks, "cec_verify_batch");
    if (st != CEC_OK) return st;
    if (!expected || !ok) return CEC_ERR_INVALID_ARGUMENT;
    if (b->n_parts == 0 || n_chunks == 0) return CEC_OK;
    const size_t n = b->n_parts * n_chunks;
    if (present) standin_check_device_range(present, n, "cec_verify_batch present");
    standin_check_device_range(expected, n * 32, "cec_verify_batch expected");
    standin_check_device_range(ok, n, "cec_verify_batch ok");
    const cec_part_batch bb = *b;
    auto fn = [=] {
        uint8_t h[32];
        for (size_t k = 0; k < bb.n_parts; ++k)
            for (size_t c = 0; c < n_chunks; ++c) {
                const size_t x = k * n_chunks + c;
                if (present && !present[x]) {
                    ok[x] = 0;
                    continue;
                }
                or_sha256(bb.base + k * bb.part_stride + (first_chunk + c) * bb.chunk_stride,
                          bb.chunk_len, h);
                ok[x] = std::memcmp(h, expected + x * 32, 32) == 0;
            }
    };
    std::vector<const void*> uses{bb.base, expected, ok};
    if (present) uses.push_back(present);
    return queued(standin_enqueue(static_cast<hipStream_t>(stream), "verify", fn, uses), "verify");
}

int cec_reconstruct_batch(const cec_codec* c, const cec_part_batch* b, const uint8_t* present,
                          int data_only, void* stream) {
    if (!c || !present) return CEC_ERR_INVALID_ARGUMENT;
    const size_t d = c->d, p = c->p, t = d + p;
    const int st = batch_ok(b, t, "cec_reconstruct_batch");
    if (st != CEC_OK || b->n_parts == 0) return st;
    bool any = false;
    for (size_t k = 0; k < b->n_parts; ++k) {
        size_t have = 0;
        for (size_t i = 0; i < t; ++i) have += present[k * t + i] ? 1 : 0;
        if (have < d) {
            g_error = "reconstruct: a part with fewer than d chunks present";
            return CEC_TOO_FEW_SHARDS_PRESENT;  // nothing launched
        }
        any |= have < t;
    }
    if (!any) return CEC_OK;
    const std::vector<uint8_t> mask(present, present + b->n_parts * t);  // read during the call
    const cec_part_batch bb = *b;
    auto fn = [=] {
        std::vector<uint8_t*> sh(t);
        const std::vector<size_t> lens(t, bb.chunk_len);
        std::vector<uint8_t> pr(t);
        for (size_t k = 0; k < bb.n_parts; ++k) {
            for (size_t i = 0; i < t; ++i) {
                sh[i] = bb.base + k * bb.part_stride + i * bb.chunk_stride;
                pr[i] = mask[k * t + i] ? 1 : 0;
            }
            (void)or_rs_reconstruct(d, p, sh.data(), lens.data(), pr.data(), t, data_only);
        }
    };
    return queued(standin_enqueue(static_cast<hipStream_t>(stream), "reconstruct", fn, {bb.base}),
                  "reconstruct");
}

}  // extern "C"

namespace cec {

hipError_t launch_move_chunks(const MoveParams& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if (!a.batch || !a.packed || !a.ids || a.t == 0 || a.len == 0) return hipErrorInvalidValue;
    standin_check_device_range(a.ids, a.n * sizeof(uint32_t), "move_chunks ids");
    if (a.packed_ids)
        standin_check_device_range(a.packed_ids, a.n * sizeof(uint32_t), "move_chunks packed_ids");
    else
        standin_check_device_range(a.packed, a.n * a.len, "move_chunks packed");
    const MoveParams m = a;
    auto fn = [=] {
        for (uint32_t j = 0; j < m.n; ++j) {
            const uint32_t id = m.ids[j];
            uint8_t* bp = m.batch + (id / m.t) * m.part_stride + (id % m.t) * m.chunk_stride;
            uint8_t* pp = m.packed + size_t(m.packed_ids ? m.packed_ids[j] : j) * m.len;
            // the ids are data: a wrong one must be a finding, not a write out of bounds
            standin_check_device_range(bp, m.len, "move_chunks batch chunk");
            standin_check_device_range(pp, m.len, "move_chunks packed chunk");
            if (m.to_batch) std::memcpy(bp, pp, m.len);
            else std::memcpy(pp, bp, m.len);
        }
    };
    return standin_enqueue(s, "move_chunks", fn, {m.batch, m.packed, m.ids});
}

hipError_t launch_carry_stash(const CarryStashParams& a, hipStream_t s) {
    if (a.n_parts == 0) return hipSuccess;
    if (!a.batch || !a.pool || !a.present || !a.ok || !a.map || (a.n_reserved && !a.reserved))
        return hipErrorInvalidValue;
    standin_check_device_range(a.present, size_t(a.n_parts) * a.t, "carry_stash present");
    standin_check_device_range(a.ok, size_t(a.n_parts) * a.t, "carry_stash ok");
    standin_check_device_range(a.map, a.n_parts * sizeof(int32_t), "carry_stash map");
    if (a.n_reserved)
        standin_check_device_range(a.reserved, a.n_reserved * sizeof(uint32_t),
                                   "carry_stash reserved");
    const CarryStashParams c = a;
    auto fn = [=] {
        uint32_t next = 0;
        for (uint32_t k = 0; k < c.n_parts; ++k) {
            auto verified = [&](uint32_t i) {
                const uint8_t f = c.present[k * c.t + i];
                return f == CEC_PRESENT_VERIFIED || (f && c.ok[k * c.t + i]);
            };
            uint32_t v = 0;
            for (uint32_t i = 0; i < c.t; ++i) v += verified(i) ? 1 : 0;
            c.map[k] = -1;
            if (v == 0 || v >= c.d || next >= c.n_reserved) continue;
            const uint32_t e = c.reserved[next++];
            c.map[k] = int32_t(e);
            for (uint32_t i = 0; i < c.t; ++i) {
                if (!verified(i)) continue;
                uint8_t* to = c.pool + (size_t(e) * c.t + i) * c.len;
                standin_check_device_range(to, c.len, "carry_stash pool chunk");
                std::memcpy(to, c.batch + k * c.part_stride + i * c.chunk_stride, c.len);
            }
        }
    };
    std::vector<const void*> uses{c.batch, c.pool, c.map};
    if (c.n_reserved) uses.push_back(c.reserved);
    return standin_enqueue(s, "carry_stash", fn, uses);
}

}  // namespace cec
