// segment_pipeline.cpp — host-staged segment pipeline (cec_segment_pipeline_*): the ragged write
// pipeline (ragged_pipeline.cpp, whose slots and slot steps it shares through parts_slots.hpp)
// with batches of column segments.  A part whose chunks are long goes through as segments of
// bounded length, one per batch, so that a batch's SHA-256 chain is one segment long, and the
// midstates of the parts under way stay in a device pool between batches (cec_encode_hash_segments,
// ragged.cpp segments_launch).
//
// Ordering across slots: every slot has its own stream and the chain of one chunk runs through
// successive slots, so every batch's resume launch waits for an event recorded behind the previous
// batch's resume launch: always, not only when the batch holds a continuation, since a reused id's
// FIRST must not overtake its previous owner's LAST.  The copies stay unordered between slots:
// H2D and D2H still overlap the kernels.  One thread drives a pipeline.
#include <algorithm>

#include "parts_slots.hpp"

using namespace cec;

struct cec_segment_pipeline : PartsSlots {
    plan::OpenIds open;
    uint8_t* midstates = nullptr;  // device: max_open * t records
    std::vector<hipEvent_t> hashed;  // per slot: behind its batch's resume launch
    hipEvent_t last_hashed = nullptr;  // the previous batch's (null: none queued yet)

    ~cec_segment_pipeline() {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return;
        (void)hipSetDevice(device);
        for (PartsSlot& s : slots)  // before anything the streams use goes away
            if (s.stream) (void)hipStreamSynchronize(s.stream);
        for (hipEvent_t e : hashed)
            if (e) (void)hipEventDestroy(e);
        if (midstates) (void)hipFree(midstates);
        (void)hipSetDevice(cur);
    }
};

extern "C" {

int cec_segment_pipeline_new(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts,
                             size_t depth, size_t max_open, cec_segment_pipeline** out) {
    if (!codec || !out) return CEC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    size_t dig = 0, records = 0, pool = 0;
    CEC_TRY(PartsSlots::check_sizes(codec, slot_data_bytes, max_parts, depth,
                                    "cec_segment_pipeline", &dig));
    if (__builtin_mul_overflow(max_open, codec->d + codec->p, &records) ||
        records > 0xFFFFFFFFull || __builtin_mul_overflow(records, plan::kMidstateBytes, &pool)) {
        set_last_error("cec_segment_pipeline_new: max_open * (d + p) records exceed 32 bits");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    if (cec_device_count() <= 0) return CEC_ERR_NO_DEVICE;
    auto* pl = new cec_segment_pipeline();
    int st = pl->make(codec, slot_data_bytes, max_parts, depth,
                      plan::segment_words(codec->d + codec->p, max_parts).bytes,
                      "cec_segment_pipeline");
    hipError_t e = hipSuccess;
    if (st == CEC_OK) {
        pl->open = plan::OpenIds(max_open);
        pl->hashed.assign(depth, nullptr);
        for (hipEvent_t& ev : pl->hashed)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess && pool) e = hipMalloc(reinterpret_cast<void**>(&pl->midstates), pool);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st = hip_fail(e, "cec_segment_pipeline_new allocation");
        }
    }
    if (st != CEC_OK) {
        delete pl;
        return st;
    }
    *out = pl;
    return CEC_OK;
}

void cec_segment_pipeline_free(cec_segment_pipeline* pl) { delete pl; }

size_t cec_segment_pipeline_depth(const cec_segment_pipeline* pl) {
    return pl ? pl->slots.size() : 0;
}

int cec_segment_pipeline_acquire(cec_segment_pipeline* pl, size_t* slot) {
    uint8_t* data = nullptr;  // the engine packs: the data region is its own
    if (!pl || !slot) return CEC_ERR_INVALID_ARGUMENT;
    return pl->acquire(slot, &data);
}

int cec_segment_pipeline_submit_from(cec_segment_pipeline* pl, size_t slot,
                                     const uint8_t* const* data_bufs, const size_t* lengths,
                                     const size_t* seg_offsets, const size_t* seg_lens,
                                     const uint32_t* open_ids, size_t n, size_t* chunksizes) {
    if (!pl || slot >= pl->slots.size() ||
        (n && (!data_bufs || !lengths || !seg_offsets || !seg_lens || !open_ids || !chunksizes)) ||
        n > pl->max_parts)
        return CEC_ERR_INVALID_ARGUMENT;
    PartsSlot& s = pl->slots[slot];
    for (size_t k = 0; k < n; ++k)
        if (lengths[k] == 0 || seg_lens[k] == 0) return CEC_EMPTY_SHARD;
    for (size_t k = 0; k < n; ++k)
        if (!data_bufs[k]) return CEC_ERR_INVALID_ARGUMENT;
    std::vector<size_t> L(n);
    for (size_t k = 0; k < n; ++k) L[k] = (lengths[k] - 1) / pl->d + 1;
    std::vector<uint8_t> flags(n);
    static const char* const kRule[] = {
        "",
        "an id is not below max_open",
        "an id is named twice in one batch",
        "a first segment on an id that is open",
        "a continuation on an id that is not open",
        "a continuation that does not start at the columns already submitted",
        "a column range past the chunk length",
        "a segment that is not the last has a length that is no multiple of 64"};
    if (const int rule = pl->open.check(L.data(), seg_offsets, seg_lens, open_ids, n, flags.data())) {
        set_last_error(std::string("cec_segment_pipeline_submit_from: ") + kRule[rule]);
        return CEC_ERR_INVALID_ARGUMENT;
    }
    size_t data_bytes = 0, parity_bytes = 0;
    CEC_TRY(pl->place(s, seg_lens, n, &data_bytes, &parity_bytes));
    CEC_TRY(pl->finish(s));  // the packing overwrites what its last batch's upload reads
    s.n_parts = 0;
    if (n == 0) return CEC_OK;
    pack_parts(s.h_data, s.doffs.data(), pl->d, data_bufs, lengths, L.data(), n, seg_offsets,
               seg_lens);
    std::copy(L.begin(), L.end(), chunksizes);
    const int st = pl->queue_or_clear(s, seg_lens, n, data_bytes, parity_bytes, [&](PartsSlot& q) {
        const hipEvent_t mine = pl->hashed[slot];
        CEC_TRY(segments_launch(pl->codec, q.d_data, q.doffs.data(), q.d_parity, q.poffs.data(),
                                q.lens.data(), n, open_ids, flags.data(), pl->midstates, q.d_dig,
                                q.stream, q.h_words, q.d_words, pl->last_hashed, mine));
        pl->last_hashed = mine;
        return int(CEC_OK);
    });
    if (st == CEC_OK) pl->open.commit(L.data(), seg_offsets, seg_lens, open_ids, flags.data(), n);
    return st;
}

int cec_segment_pipeline_wait(cec_segment_pipeline* pl, size_t slot, const uint8_t** parity,
                              const uint8_t** digests, size_t* n) {
    return pl ? pl->wait(slot, parity, digests, n) : CEC_ERR_INVALID_ARGUMENT;
}

int cec_segment_pipeline_query(cec_segment_pipeline* pl, size_t slot) {
    return pl ? pl->query(slot) : CEC_ERR_INVALID_ARGUMENT;
}

int cec_segment_pipeline_drain(cec_segment_pipeline* pl) {
    return pl ? pl->drain() : CEC_ERR_INVALID_ARGUMENT;
}

size_t cec_segment_pipeline_open_count(const cec_segment_pipeline* pl) {
    return pl ? pl->open.count : 0;
}

int cec_segment_pipeline_abandon(cec_segment_pipeline* pl, uint32_t id) {
    return pl && pl->open.abandon(id) ? CEC_OK : CEC_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
