// scrub_pipeline.cpp — host-staged scrub pipeline (cec_scrub_pipeline_*): cec_parts_verify with
// slots in flight, whose batches carry segments of stored copies.  A long copy goes through as
// segments of bounded length, one per batch, so that a batch's SHA-256 chain is one segment long,
// and the midstates of the copies under way stay in a device pool between batches
// (cec_verify_segments, ragged.cpp verify_segments_launch).  There is no codec: a scrub decodes
// nothing.
//
// A slot is one page-locked and one device staging of the same layout, [the batch's pieces, packed
// 16-byte aligned (cec_ragged_layout with one chunk per part)][the launch words, the expected rows
// among them][the ok bytes], so that everything a batch sends goes up in one copy and only the ok
// bytes come back; plus one non-blocking stream and two events.  All of it is made when the
// pipeline is made and never later (ragged_pipeline.cpp says why).
//
// Ordering across slots, as in segment_pipeline.cpp: every slot has its own stream and the chain of
// one copy runs through successive slots, so every batch's launch waits for an event recorded
// behind the previous batch's: always, not only when the batch holds a continuation, since a
// reused id's FIRST must not overtake its previous owner's LAST.  The copies stay unordered
// between slots.  One thread drives a pipeline.
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"
#include "hostmem.hpp"

using namespace cec;

namespace {

struct ScrubSlot {
    uint8_t *h = nullptr, *d = nullptr;  // the staging: page-locked, device
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;    // behind the batch's copy back
    hipEvent_t hashed = nullptr;  // behind the batch's launch
    bool in_flight = false;
    size_t n = 0;       // the batch's entries (0: nothing valid on the slot)
    size_t ok_off = 0;  // where its ok bytes lie in the staging
};

}  // namespace

struct cec_scrub_pipeline {
    int device = 0;
    size_t slot_bytes = 0, max_entries = 0, stage_bytes = 0;
    std::vector<ScrubSlot> slots;
    size_t next = 0;
    plan::OpenIds open;
    uint8_t* midstates = nullptr;      // device: max_open records
    hipEvent_t last_hashed = nullptr;  // the previous batch's (null: none queued yet)

    cec_scrub_pipeline() = default;
    cec_scrub_pipeline(const cec_scrub_pipeline&) = delete;
    cec_scrub_pipeline& operator=(const cec_scrub_pipeline&) = delete;

    ~cec_scrub_pipeline() {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return;
        (void)hipSetDevice(device);
        for (ScrubSlot& s : slots)  // before anything the streams use goes away
            if (s.stream) (void)hipStreamSynchronize(s.stream);
        for (ScrubSlot& s : slots) {
            if (s.done) (void)hipEventDestroy(s.done);
            if (s.hashed) (void)hipEventDestroy(s.hashed);
            if (s.stream) (void)hipStreamDestroy(s.stream);
            if (s.d) (void)hipFree(s.d);
            if (s.h) (void)hipHostFree(s.h);
        }
        if (midstates) (void)hipFree(midstates);
        (void)hipSetDevice(cur);
    }

    // Every allocation, on the current device.  On failure the object is left for its destructor.
    int make(size_t depth, size_t pool_bytes) {
        hipError_t e = hipGetDevice(&device);
        if (e == hipSuccess) slots.resize(depth);
        for (ScrubSlot& s : slots) {
            if (e == hipSuccess)
                e = host_malloc_near(reinterpret_cast<void**>(&s.h), stage_bytes,
                                     hipHostMallocDefault, device);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s.d), stage_bytes);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s.hashed, hipEventDisableTiming);
        }
        if (e == hipSuccess && pool_bytes)
            e = hipMalloc(reinterpret_cast<void**>(&midstates), pool_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return hip_fail(e, "cec_scrub_pipeline_new allocation");
        }
        return CEC_OK;
    }

    int finish(ScrubSlot& s) {  // waits for the slot's batch, if one is in flight
        if (s.in_flight) {
            HIP_TRY(hipEventSynchronize(s.done));
            s.in_flight = false;
        }
        return CEC_OK;
    }

    // Queue the packed batch: the one upload and the launch (verify_segments_launch), the copy back
    // of the ok bytes, the event.
    int queue(ScrubSlot& s, const size_t* offs, const size_t* seg_lens, size_t n,
              size_t data_bytes, const uint32_t* ids, const uint8_t* flags) {
        OnDevice guard(device);
        HIP_TRY(guard.status());
        const ScrubStage stage{s.h, s.d, data_bytes};
        const plan::ScrubWords w = plan::scrub_words(n);
        CEC_TRY(verify_segments_launch(s.d, offs, seg_lens, n, ids, flags, midstates, nullptr,
                                       nullptr, s.stream, &stage, last_hashed, s.hashed));
        last_hashed = s.hashed;
        s.ok_off = data_bytes + w.ok.off;
        HIP_TRY(hipMemcpyAsync(s.h + s.ok_off, s.d + s.ok_off, n, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipEventRecord(s.done, s.stream));
        s.in_flight = true;
        s.n = n;
        return CEC_OK;
    }
};

extern "C" {

int cec_scrub_pipeline_new(size_t slot_bytes, size_t max_entries, size_t depth, size_t max_open,
                           cec_scrub_pipeline** out) {
    if (!out) return CEC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    size_t stage = 0, pool = 0;
    if (depth == 0 || depth > 16 || max_entries == 0 || max_entries > 0xFFFFFFFFull ||
        slot_bytes < 16 || slot_bytes > SIZE_MAX - 16 ||
        __builtin_add_overflow(round_up(slot_bytes, 16), plan::scrub_words(max_entries).bytes,
                               &stage)) {
        set_last_error("cec_scrub_pipeline_new: depth 1..16, max_entries 1..2^32-1, slot_bytes >= "
                       "16, sizes within size_t");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    if (max_open > 0xFFFFFFFFull || __builtin_mul_overflow(max_open, plan::kMidstateBytes, &pool)) {
        set_last_error("cec_scrub_pipeline_new: max_open records exceed 32 bits");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    if (cec_device_count() <= 0) return CEC_ERR_NO_DEVICE;
    auto* pl = new cec_scrub_pipeline();
    pl->slot_bytes = slot_bytes;
    pl->max_entries = max_entries;
    pl->stage_bytes = stage;
    pl->open = plan::OpenIds(max_open);
    const int st = pl->make(depth, pool);
    if (st != CEC_OK) {
        delete pl;
        return st;
    }
    *out = pl;
    return CEC_OK;
}

void cec_scrub_pipeline_free(cec_scrub_pipeline* pl) { delete pl; }

size_t cec_scrub_pipeline_depth(const cec_scrub_pipeline* pl) { return pl ? pl->slots.size() : 0; }

// Next slot in round-robin order; waits for that slot's previous batch, after which its previous
// results are void.
int cec_scrub_pipeline_acquire(cec_scrub_pipeline* pl, size_t* slot) {
    if (!pl || !slot) return CEC_ERR_INVALID_ARGUMENT;
    const size_t i = pl->next;
    CEC_TRY(pl->finish(pl->slots[i]));
    pl->next = (pl->next + 1) % pl->slots.size();
    *slot = i;
    return CEC_OK;
}

int cec_scrub_pipeline_submit_from(cec_scrub_pipeline* pl, size_t slot, const uint8_t* const* bufs,
                                   const size_t* lens, const size_t* seg_offsets,
                                   const size_t* seg_lens, const uint32_t* open_ids,
                                   const uint8_t* expected, size_t n) {
    if (!pl || slot >= pl->slots.size() ||
        (n && (!bufs || !lens || !seg_offsets || !seg_lens || !open_ids || !expected)) ||
        n > pl->max_entries)
        return CEC_ERR_INVALID_ARGUMENT;
    ScrubSlot& s = pl->slots[slot];
    for (size_t k = 0; k < n; ++k)
        if (lens[k] == 0 || seg_lens[k] == 0) return CEC_EMPTY_SHARD;
    for (size_t k = 0; k < n; ++k)
        if (!bufs[k]) return CEC_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> flags(n);
    static const char* const kRule[] = {
        "",
        "an id is not below max_open",
        "an id is named twice in one batch",
        "a first segment on an id that is open",
        "a continuation on an id that is not open",
        "a continuation that does not start at the bytes already submitted",
        "a range past the copy's length",
        "a segment that is not the last has a length that is no multiple of 64"};
    if (const int rule = pl->open.check(lens, seg_offsets, seg_lens, open_ids, n, flags.data())) {
        set_last_error(std::string("cec_scrub_pipeline_submit_from: ") + kRule[rule]);
        return CEC_ERR_INVALID_ARGUMENT;
    }
    std::vector<size_t> offs(n);
    size_t data_bytes = 0;
    CEC_TRY(ragged_layout(1, seg_lens, n, offs.data(), &data_bytes));
    if (data_bytes > pl->slot_bytes) {
        set_last_error("cec_scrub_pipeline_submit_from: the batch's padded segments exceed "
                       "slot_bytes");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    CEC_TRY(pl->finish(s));  // the packing overwrites what its last batch's upload reads
    s.n = 0;
    if (n == 0) return CEC_OK;
    // a copy is a part of one chunk: piece 0 = its bytes [seg_offsets[k], + seg_lens[k])
    pack_parts(s.h, offs.data(), 1, bufs, lens, lens, n, seg_offsets, seg_lens);
    // the expected rows of the entries that end a chain, into the words that go up
    const plan::ScrubWords w = plan::scrub_words(n);
    const plan::View v{s.h + data_bytes, s.d + data_bytes};
    plan::DigestRow* rows = v.host(w.expected);
    for (size_t k = 0; k < n; ++k)
        if (flags[k] & plan::kSegLast) std::memcpy(rows[k].b, expected + k * 32, 32);
    const int st = pl->queue(s, offs.data(), seg_lens, n, data_bytes, open_ids, flags.data());
    if (st != CEC_OK) {  // a failed queue leaves nothing of it in flight and the slot usable
        const std::string why = last_error();
        (void)hipStreamSynchronize(s.stream);
        (void)hipGetLastError();
        set_last_error(why);
        return st;
    }
    pl->open.commit(lens, seg_offsets, seg_lens, open_ids, flags.data(), n);
    return CEC_OK;
}

int cec_scrub_pipeline_wait(cec_scrub_pipeline* pl, size_t slot, const uint8_t** ok, size_t* n) {
    if (!pl || slot >= pl->slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    ScrubSlot& s = pl->slots[slot];
    CEC_TRY(pl->finish(s));
    if (ok) *ok = s.h + s.ok_off;
    if (n) *n = s.n;
    return CEC_OK;
}

// 1 when the slot's batch is complete (or none is in flight), 0 while it runs; never blocks.
int cec_scrub_pipeline_query(cec_scrub_pipeline* pl, size_t slot) {
    if (!pl || slot >= pl->slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    ScrubSlot& s = pl->slots[slot];
    if (!s.in_flight) return 1;
    const hipError_t e = hipEventQuery(s.done);
    (void)hipGetLastError();
    return e == hipErrorNotReady ? 0 : 1;
}

int cec_scrub_pipeline_drain(cec_scrub_pipeline* pl) {
    if (!pl) return CEC_ERR_INVALID_ARGUMENT;
    for (ScrubSlot& s : pl->slots) CEC_TRY(pl->finish(s));
    return CEC_OK;
}

size_t cec_scrub_pipeline_open_count(const cec_scrub_pipeline* pl) {
    return pl ? pl->open.count : 0;
}

int cec_scrub_pipeline_abandon(cec_scrub_pipeline* pl, uint32_t id) {
    return pl && pl->open.abandon(id) ? CEC_OK : CEC_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
