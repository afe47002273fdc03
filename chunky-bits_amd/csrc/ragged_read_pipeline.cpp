// ragged_read_pipeline.cpp — host-staged ragged read pipeline (cec_parts_reader_*): cec_parts_read
// with slots in flight and a packed return.  A batch is a set of parts of different chunk lengths
// in the ragged layout (cec_ragged_layout); its loaded chunks go up at their offsets, the device
// verifies, plans and rebuilds (ragged.cpp read_ragged_async), gathers what it rebuilt into the
// slot's dense return region (plan_kernels.hip), and only that region comes back.
//
// A reader owns `depth` slots on one GPU.  A slot has pinned and device regions for the batch, the
// return region, the digests, flags, statuses and offsets, one non-blocking stream and one event,
// all made when the reader is made and never later (ragged_pipeline.cpp and pipeline.cpp
// slot_stream explain why).  The per-call words of the packed read come from the scratch pool,
// which hands the same buffers out again once a slot's batch is done.  Everything of a batch is
// queued on the slot's stream, so the packing of one slot (submit_from, host threads) overlaps the
// copies and SHA-256 chains of the others and the caller's use of finished ones.  One thread
// drives a reader.
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"
#include "chunky_ec_parts_read.h"
#include "hostmem.hpp"

using namespace cec;

namespace {

struct ReadSlot {
    uint8_t *h_stage = nullptr, *h_exp = nullptr, *h_ret = nullptr, *h_ver = nullptr;  // pinned
    int* h_status = nullptr;                                                           // pinned
    size_t* h_off = nullptr;                                                           // pinned
    uint8_t *d_base = nullptr, *d_exp = nullptr, *d_ret = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool in_flight = false;
    size_t n_parts = 0;
    size_t fetched = 0;  // bytes of the return region that are (or are on their way) in h_ret
    std::vector<size_t> lens, offs;  // this batch's layout
    std::vector<uint8_t> present;    // and its loaded flags
};

}  // namespace

struct cec_parts_reader {
    cec_codec* codec = nullptr;
    int device = 0;
    size_t d = 0, p = 0, t = 0, rows = 0, cap = 0, ret_cap = 0, max_parts = 0;
    bool data_only = false;
    std::vector<ReadSlot> slots;
    size_t next = 0;
    uint64_t bytes_up = 0, bytes_down = 0, tail_copies = 0;

    ~cec_parts_reader() {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return;
        (void)hipSetDevice(device);
        for (ReadSlot& s : slots) {
            if (s.stream) (void)hipStreamSynchronize(s.stream);
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.stream) (void)hipStreamDestroy(s.stream);
            for (uint8_t* ptr : {s.d_base, s.d_exp, s.d_ret})
                if (ptr) (void)hipFree(ptr);
            for (void* ptr : {static_cast<void*>(s.h_stage), static_cast<void*>(s.h_exp),
                              static_cast<void*>(s.h_ret), static_cast<void*>(s.h_ver),
                              static_cast<void*>(s.h_status), static_cast<void*>(s.h_off)})
                if (ptr) (void)hipHostFree(ptr);
        }
        (void)hipSetDevice(cur);
    }

    int finish(ReadSlot& s) {
        if (s.in_flight) {
            HIP_TRY(hipEventSynchronize(s.done));
            s.in_flight = false;
        }
        return CEC_OK;
    }

    // Every check of a submit's arguments behind the shards (no device use).
    int check(size_t slot, const size_t* lens, size_t n, const uint8_t* present,
              const uint8_t* expected) const {
        if (slot >= slots.size() || (n && (!lens || !present || !expected)) || n > max_parts)
            return CEC_ERR_INVALID_ARGUMENT;
        for (size_t k = 0; k < n; ++k)
            if (lens[k] == 0) return CEC_EMPTY_SHARD;
        return CEC_OK;
    }

    // The layout of a batch of these (nonzero) chunk lengths in the slot (no device use).
    int place(const size_t* lens, size_t n, std::vector<size_t>* offs) const {
        offs->resize(n);
        size_t total = 0;
        CEC_TRY(ragged_layout(t, lens, n, offs->data(), &total));
        if (total > cap) {
            set_last_error("cec_parts_reader: the batch's layout exceeds slot_bytes");
            return CEC_ERR_INVALID_ARGUMENT;
        }
        return CEC_OK;
    }

    // Queue the placed batch whose loaded chunks lie in the slot's staging.
    int queue(ReadSlot& s, const size_t* lens, size_t n, const uint8_t* present,
              const uint8_t* expected) {
        OnDevice guard(device);
        HIP_TRY(guard.status());
        CEC_TRY(finish(s));  // its regions may still be read by its last batch
        s.n_parts = 0;       // nothing valid on the slot until this batch is queued
        s.fetched = 0;
        s.lens.assign(lens, lens + n);
        s.present.assign(present, present + n * t);
        std::memcpy(s.h_exp, expected, n * t * 32);
        Spans spans;
        const size_t up =
            n * t * 32 + plan::loaded_spans(t, lens, s.offs.data(), n, present, &spans);
        const size_t guess = plan::return_guess(d, t, lens, n, present, data_only);
        HIP_TRY(hipMemcpyAsync(s.d_exp, s.h_exp, n * t * 32, hipMemcpyHostToDevice, s.stream));
        CEC_TRY(copy_spans(s.h_stage, s.d_base, spans, true, s.stream));
        CEC_TRY(cec_read_ragged_packed_async(codec, s.d_base, s.offs.data(), s.lens.data(), n,
                                             s.present.data(), s.d_exp, data_only ? 1 : 0, s.h_ver,
                                             s.h_status, s.d_ret, ret_cap, s.h_off, s.stream));
        // at most the worst case, which the region holds (new's ret_cap)
        if (guess) HIP_TRY(hipMemcpyAsync(s.h_ret, s.d_ret, guess, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipEventRecord(s.done, s.stream));
        s.in_flight = true;
        s.n_parts = n;
        s.fetched = guess;
        bytes_up += up;
        bytes_down += guess;
        return CEC_OK;
    }

    // A failed queue leaves nothing of it in flight and the slot usable.
    int queue_or_clear(ReadSlot& s, const size_t* lens, size_t n, const uint8_t* present,
                       const uint8_t* expected) {
        const int st = queue(s, lens, n, present, expected);
        if (st != CEC_OK && s.stream) {
            const std::string why = last_error();
            (void)hipStreamSynchronize(s.stream);
            (void)hipGetLastError();
            set_last_error(why);
        }
        return st;
    }

    // What the device rebuilt beyond the host's guess: one more copy, waited for.
    int fetch_tail(ReadSlot& s) {
        const size_t total = s.n_parts ? s.h_off[s.n_parts] : 0;
        if (total <= s.fetched) return CEC_OK;
        if (total > ret_cap) {  // cannot happen: the packed read's bound
            set_last_error("cec_parts_reader_wait: the return exceeds the slot's region");
            return CEC_ERR_HIP;
        }
        OnDevice guard(device);
        HIP_TRY(guard.status());
        HIP_TRY(hipMemcpyAsync(s.h_ret + s.fetched, s.d_ret + s.fetched, total - s.fetched,
                               hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        bytes_down += total - s.fetched;
        ++tail_copies;
        s.fetched = total;
        return CEC_OK;
    }

    // fn(item, where its bytes lie in h_ret, L) for every rebuilt chunk of a waited batch.
    template <typename Fn>
    void rebuilt_chunks(const ReadSlot& s, Fn fn) const {
        for (size_t k = 0; k < s.n_parts; ++k) {
            if (s.h_status[k] != CEC_OK) continue;
            const size_t L = s.lens[k], cs = ragged_stride(L);
            size_t r = 0;
            for (size_t i = 0; i < t; ++i)
                if (!s.h_ver[k * t + i] && fills_slot(i, d, data_only))
                    fn(k * t + i, s.h_off[k] + (r++) * cs, L);
        }
    }
};

extern "C" {

int cec_parts_reader_new(const cec_codec* codec, size_t slot_bytes, size_t max_parts, size_t depth,
                         int data_only, cec_parts_reader** out) {
    if (!codec || !out) return CEC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    const size_t d = codec->d, p = codec->p, t = d + p;
    const size_t rows = data_only ? std::min(p, d) : p;
    size_t need = 0, items = 0, dig = 0, ret_cap = 0;
    if (depth == 0 || depth > 16 || max_parts == 0 || __builtin_mul_overflow(t, size_t(16), &need) ||
        slot_bytes < need || slot_bytes > SIZE_MAX - 16 ||
        __builtin_mul_overflow(max_parts, t, &items) || items > 0xFFFFFFFFull ||
        __builtin_mul_overflow(items, size_t(32), &dig) ||
        __builtin_mul_overflow(slot_bytes / t, rows, &ret_cap) || ret_cap > SIZE_MAX - rows * 16 ||
        max_parts > (SIZE_MAX - 8) / 8) {
        set_last_error("cec_parts_reader_new: depth 1..16, max_parts >= 1, slot_bytes >= "
                       "(d + p) * 16, sizes within size_t");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    if (d > 0xFFFFFFFFull || p > 0xFFFFFFFFull || !decode_plan_covers(uint32_t(d), uint32_t(p))) {
        set_last_error("cec_parts_reader_new: the device planner covers d <= 32 and p <= 8; use "
                       "cec_parts_read for this shape");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    if (cec_device_count() <= 0) return CEC_ERR_NO_DEVICE;
    auto* rd = new cec_parts_reader();
    rd->codec = const_cast<cec_codec*>(codec);
    rd->d = d;
    rd->p = p;
    rd->t = t;
    rd->rows = rows;
    rd->data_only = data_only != 0;
    rd->cap = slot_bytes;
    // a batch whose layout fits the slot has strides that sum to at most slot_bytes / t, and every
    // part returns at most `rows` of them; the slack keeps the bound whatever the rounding
    rd->ret_cap = ret_cap + rows * 16;
    rd->max_parts = max_parts;
    hipError_t e = hipGetDevice(&rd->device);
    uint8_t* mat = nullptr;  // the codec's matrix on this device: made now, not mid-stream
    int st = e == hipSuccess ? rd->codec->matrix_device(&mat) : CEC_OK;
    if (e == hipSuccess && st == CEC_OK) rd->slots.resize(depth);
    for (ReadSlot& s : rd->slots) {
        auto host = [&](auto** ptr, size_t bytes) {  // pinned, on the device's NUMA node
            if (e == hipSuccess)
                e = host_malloc_near(reinterpret_cast<void**>(ptr), bytes, hipHostMallocDefault,
                                     rd->device);
        };
        auto dev = [&](uint8_t** ptr, size_t bytes) {
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(ptr), bytes);
        };
        host(&s.h_stage, round_up(rd->cap, 16));
        host(&s.h_exp, dig);
        host(&s.h_ret, rd->ret_cap);
        host(&s.h_ver, items);
        host(&s.h_status, max_parts * sizeof(int));
        host(&s.h_off, (max_parts + 1) * sizeof(size_t));
        dev(&s.d_base, round_up(rd->cap, 16));
        dev(&s.d_exp, dig);
        dev(&s.d_ret, rd->ret_cap);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        s.lens.reserve(max_parts);
        s.offs.reserve(max_parts);
        s.present.reserve(items);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess || st != CEC_OK) {
        delete rd;
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return hip_fail(e, "cec_parts_reader_new allocation");
        }
        return st;
    }
    *out = rd;
    return CEC_OK;
}

void cec_parts_reader_free(cec_parts_reader* rd) { delete rd; }

size_t cec_parts_reader_depth(const cec_parts_reader* rd) { return rd ? rd->slots.size() : 0; }

int cec_parts_reader_acquire(cec_parts_reader* rd, size_t* slot, uint8_t** stage) {
    if (!rd || !slot || !stage) return CEC_ERR_INVALID_ARGUMENT;
    const size_t i = rd->next;
    ReadSlot& s = rd->slots[i];
    CEC_TRY(rd->finish(s));
    rd->next = (rd->next + 1) % rd->slots.size();
    *slot = i;
    *stage = s.h_stage;
    return CEC_OK;
}

int cec_parts_reader_submit(cec_parts_reader* rd, size_t slot, const size_t* chunk_lens,
                            size_t n_parts, const uint8_t* present, const uint8_t* expected) {
    if (!rd) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(rd->check(slot, chunk_lens, n_parts, present, expected));
    ReadSlot& s = rd->slots[slot];
    std::vector<size_t> offs;
    CEC_TRY(rd->place(chunk_lens, n_parts, &offs));
    if (n_parts == 0) {  // a batch of nothing
        CEC_TRY(rd->finish(s));
        s.n_parts = 0;
        return CEC_OK;
    }
    s.offs.swap(offs);
    return rd->queue_or_clear(s, chunk_lens, n_parts, present, expected);
}

int cec_parts_reader_submit_from(cec_parts_reader* rd, size_t slot, const uint8_t* const* shards,
                                 const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                                 const uint8_t* expected) {
    if (!rd || (n_parts && !shards)) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(rd->check(slot, chunk_lens, n_parts, present, expected));
    CEC_TRY(null_slot_rule("cec_parts_reader_submit_from", shards, present, n_parts, rd->d, rd->t,
                           rd->data_only));
    ReadSlot& s = rd->slots[slot];
    std::vector<size_t> offs;
    CEC_TRY(rd->place(chunk_lens, n_parts, &offs));
    CEC_TRY(rd->finish(s));  // the packing overwrites what its last batch's upload reads
    s.n_parts = 0;
    if (n_parts == 0) return CEC_OK;
    s.offs.swap(offs);
    pack_loaded(s.h_stage, s.offs.data(), rd->t, shards, chunk_lens, n_parts, present);
    return rd->queue_or_clear(s, chunk_lens, n_parts, present, expected);
}

int cec_parts_reader_wait(cec_parts_reader* rd, size_t slot, const uint8_t** verified,
                          const int** part_status, const uint8_t** rebuilt,
                          const size_t** rebuilt_offsets, size_t* n_parts) {
    if (!rd || slot >= rd->slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    ReadSlot& s = rd->slots[slot];
    CEC_TRY(rd->finish(s));
    CEC_TRY(rd->fetch_tail(s));
    if (s.n_parts == 0) s.h_off[0] = 0;
    if (verified) *verified = s.h_ver;
    if (part_status) *part_status = s.h_status;
    if (rebuilt) *rebuilt = s.h_ret;
    if (rebuilt_offsets) *rebuilt_offsets = s.h_off;
    if (n_parts) *n_parts = s.n_parts;
    return CEC_OK;
}

int cec_parts_reader_scatter(cec_parts_reader* rd, size_t slot, uint8_t* const* shards) {
    if (!rd || slot >= rd->slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    ReadSlot& s = rd->slots[slot];
    if (s.n_parts == 0) return CEC_OK;
    if (!shards) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(null_slot_rule("cec_parts_reader_scatter", shards, s.present.data(), s.n_parts, rd->d,
                           rd->t, rd->data_only));
    CEC_TRY(rd->finish(s));
    CEC_TRY(rd->fetch_tail(s));
    rd->rebuilt_chunks(s, [&](size_t item, size_t at, size_t L) {
        std::memcpy(shards[item], s.h_ret + at, L);
    });
    return CEC_OK;
}

int cec_parts_reader_query(cec_parts_reader* rd, size_t slot) {
    if (!rd || slot >= rd->slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    ReadSlot& s = rd->slots[slot];
    if (!s.in_flight) return 1;
    const hipError_t e = hipEventQuery(s.done);
    (void)hipGetLastError();
    return e == hipErrorNotReady ? 0 : 1;
}

int cec_parts_reader_drain(cec_parts_reader* rd) {
    if (!rd) return CEC_ERR_INVALID_ARGUMENT;
    for (ReadSlot& s : rd->slots) CEC_TRY(rd->finish(s));
    return CEC_OK;
}

void cec_parts_reader_stats(const cec_parts_reader* rd, uint64_t* bytes_up, uint64_t* bytes_down,
                            uint64_t* tail_copies) {
    if (bytes_up) *bytes_up = rd ? rd->bytes_up : 0;
    if (bytes_down) *bytes_down = rd ? rd->bytes_down : 0;
    if (tail_copies) *tail_copies = rd ? rd->tail_copies : 0;
}

}  // extern "C"
