// ragged_pipeline.cpp — host-staged ragged write pipeline (cec_parts_pipeline_*): cec_parts_encode
// with slots in flight.  A batch is a set of parts of different chunk lengths in the split ragged
// layout (cec_split_layout): the data chunks of all parts in one region, their parity in another,
// so the data goes up in one copy of exactly its bytes and the parity comes back in one.
//
// A pipeline owns `depth` slots on one GPU.  A slot has pinned and device regions for data,
// parity, digests and the launches' per-part words, one non-blocking stream and one event, all
// made when the pipeline is made and never later (pipeline.cpp slot_stream: making streams while
// other queues of the process are busy deadlocked the round-5 scheduler).  H2D, the ragged encode
// and SHA-256 launches (ragged.cpp ragged_launch) and the two D2H copies are queued on the slot's
// stream, so the packing of one slot (submit_from, host threads) overlaps the copies and kernels
// of the others and the caller's use of finished ones.  One thread drives a pipeline.
#include <algorithm>

#include "hostmem.hpp"
#include "parts_slots.hpp"

using namespace cec;

// ---- The slot steps (parts_slots.hpp), shared with the segment pipeline. ----

PartsSlots::~PartsSlots() {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return;
    (void)hipSetDevice(device);
    for (PartsSlot& s : slots) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        for (uint8_t* ptr : {s.d_data, s.d_parity, s.d_dig, s.d_words})
            if (ptr) (void)hipFree(ptr);
        for (uint8_t* ptr : {s.h_data, s.h_parity, s.h_dig, s.h_words})
            if (ptr) (void)hipHostFree(ptr);
    }
    (void)hipSetDevice(cur);
}

int PartsSlots::check_sizes(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts,
                            size_t depth, const char* who, size_t* dig) {
    const size_t d = codec->d, p = codec->p, t = d + p;
    size_t need = 0, items = 0;
    if (depth == 0 || depth > 16 || max_parts == 0 || __builtin_mul_overflow(d, size_t(16), &need) ||
        slot_data_bytes < need || slot_data_bytes > SIZE_MAX - 16 ||
        __builtin_mul_overflow(max_parts, t, &items) || items > 0xFFFFFFFFull ||
        __builtin_mul_overflow(items, size_t(32), dig) ||
        __builtin_mul_overflow(slot_data_bytes / d, p, &need) || need > SIZE_MAX - p * 16) {
        set_last_error(std::string(who) + "_new: depth 1..16, max_parts >= 1, slot_data_bytes >= "
                       "d * 16, sizes within size_t");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    return CEC_OK;
}

int PartsSlots::make(const cec_codec* cc, size_t slot_data_bytes, size_t max_parts_, size_t depth,
                     size_t words, const char* who_) {
    who = who_;
    codec = const_cast<cec_codec*>(cc);
    d = codec->d;
    p = codec->p;
    t = d + p;
    data_cap = slot_data_bytes;
    // a batch of padded data D has parity D / d * p; the slack keeps the region's end past a
    // last chunk's stride whatever the rounding
    parity_cap = slot_data_bytes / d * p + p * 16;
    max_parts = max_parts_;
    const size_t dig = max_parts * t * 32;
    hipError_t e = hipGetDevice(&device);
    uint32_t* rec = nullptr;  // the codec's encode record on this device: made now, not mid-stream
    const int st = e == hipSuccess ? codec->encode_record(&rec) : CEC_OK;
    if (e == hipSuccess && st == CEC_OK) slots.resize(depth);
    for (PartsSlot& s : slots) {
        auto host = [&](uint8_t** ptr, size_t bytes) {  // pinned, on the device's NUMA node
            if (e == hipSuccess)
                e = host_malloc_near(reinterpret_cast<void**>(ptr), bytes, hipHostMallocDefault,
                                     device);
        };
        auto dev = [&](uint8_t** ptr, size_t bytes) {
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(ptr), bytes);
        };
        host(&s.h_data, round_up(data_cap, 16));
        host(&s.h_parity, parity_cap);
        host(&s.h_dig, dig);
        host(&s.h_words, words);
        dev(&s.d_data, round_up(data_cap, 16));
        dev(&s.d_parity, parity_cap);
        dev(&s.d_dig, dig);
        dev(&s.d_words, words);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        s.lens.reserve(max_parts);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(e, (std::string(who) + "_new allocation").c_str());
    }
    return st;
}

int PartsSlots::finish(PartsSlot& s) {
    if (s.in_flight) {
        HIP_TRY(hipEventSynchronize(s.done));
        s.in_flight = false;
    }
    return CEC_OK;
}

int PartsSlots::place(PartsSlot& s, const size_t* lens, size_t n, size_t* data_bytes,
                      size_t* parity_bytes) const {
    std::vector<size_t> doffs(n), poffs(n);
    CEC_TRY(split_layout(d, p, lens, n, doffs.data(), poffs.data(), data_bytes, parity_bytes));
    if (*data_bytes > data_cap) {
        set_last_error(std::string(who) + ": the batch's padded data exceeds slot_data_bytes");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    CEC_TRY(split_check(d, p, s.d_data, doffs.data(), s.d_parity, poffs.data(), lens, n));
    s.doffs.swap(doffs);
    s.poffs.swap(poffs);
    return CEC_OK;
}

int PartsSlots::queue(PartsSlot& s, const size_t* lens, size_t n, size_t data_bytes,
                      size_t parity_bytes, const Launch& launch) {
    OnDevice guard(device);
    HIP_TRY(guard.status());
    CEC_TRY(finish(s));  // its words and regions may still be read by its last batch
    s.n_parts = 0;       // nothing valid on the slot until this batch is queued
    s.lens.assign(lens, lens + n);
    HIP_TRY(hipMemcpyAsync(s.d_data, s.h_data, data_bytes, hipMemcpyHostToDevice, s.stream));
    CEC_TRY(launch(s));
    HIP_TRY(hipMemcpyAsync(s.h_parity, s.d_parity, parity_bytes, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.h_dig, s.d_dig, n * t * 32, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipEventRecord(s.done, s.stream));
    s.in_flight = true;
    s.n_parts = n;
    return CEC_OK;
}

int PartsSlots::queue_or_clear(PartsSlot& s, const size_t* lens, size_t n, size_t data_bytes,
                               size_t parity_bytes, const Launch& launch) {
    const int st = queue(s, lens, n, data_bytes, parity_bytes, launch);
    if (st != CEC_OK && s.stream) {
        const std::string why = last_error();
        (void)hipStreamSynchronize(s.stream);
        (void)hipGetLastError();
        set_last_error(why);
    }
    return st;
}

// Next slot in round-robin order; waits for that slot's previous batch, after which its previous
// results are void.  *data = the slot's pinned data region (slot_data_bytes).
int PartsSlots::acquire(size_t* slot, uint8_t** data) {
    const size_t i = next;
    PartsSlot& s = slots[i];
    CEC_TRY(finish(s));
    next = (next + 1) % slots.size();
    *slot = i;
    *data = s.h_data;
    return CEC_OK;
}

// Waits for the slot's batch (none in flight: returns at once, as cec_pipeline_wait).  *parity =
// the slot's pinned parity region: part k's parity chunk i at parity_offsets[k] + i * stride(L_k)
// of cec_split_layout, bytes between chunks unspecified; *digests = [n][d+p][32]; *n_parts = the
// batch's parts.  Valid until the slot is acquired again.
int PartsSlots::wait(size_t slot, const uint8_t** parity, const uint8_t** digests,
                     size_t* n_parts) {
    if (slot >= slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    PartsSlot& s = slots[slot];
    CEC_TRY(finish(s));
    if (parity) *parity = s.h_parity;
    if (digests) *digests = s.h_dig;
    if (n_parts) *n_parts = s.n_parts;
    return CEC_OK;
}

// 1 when the slot's batch is complete (or none is in flight), 0 while it runs; never blocks.
int PartsSlots::query(size_t slot) {
    if (slot >= slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    PartsSlot& s = slots[slot];
    if (!s.in_flight) return 1;
    const hipError_t e = hipEventQuery(s.done);
    (void)hipGetLastError();
    return e == hipErrorNotReady ? 0 : 1;
}

int PartsSlots::drain() {
    for (PartsSlot& s : slots) CEC_TRY(finish(s));
    return CEC_OK;
}

// ---- The parts pipeline. ----

struct cec_parts_pipeline : PartsSlots {
    // The batch's launches: the ragged encode and SHA-256 of whole parts (ragged.cpp).
    Launch whole_parts() {
        return [this](PartsSlot& s) {
            return ragged_launch(codec, s.d_data, s.doffs.data(), s.d_parity, s.poffs.data(),
                                 s.lens.data(), s.lens.size(), s.d_dig, s.stream, s.h_words,
                                 s.d_words);
        };
    }
};

extern "C" {

int cec_parts_pipeline_new(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts,
                           size_t depth, cec_parts_pipeline** out) {
    if (!codec || !out) return CEC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    size_t dig = 0;
    CEC_TRY(PartsSlots::check_sizes(codec, slot_data_bytes, max_parts, depth, "cec_parts_pipeline",
                                    &dig));
    if (cec_device_count() <= 0) return CEC_ERR_NO_DEVICE;
    auto* pl = new cec_parts_pipeline();
    const int st = pl->make(codec, slot_data_bytes, max_parts, depth,
                            plan::ragged_words_bytes(codec->d + codec->p, max_parts),
                            "cec_parts_pipeline");
    if (st != CEC_OK) {
        delete pl;
        return st;
    }
    *out = pl;
    return CEC_OK;
}

void cec_parts_pipeline_free(cec_parts_pipeline* pl) { delete pl; }

size_t cec_parts_pipeline_depth(const cec_parts_pipeline* pl) { return pl ? pl->slots.size() : 0; }

// Next slot in round-robin order; waits for that slot's previous batch, after which its previous
// results are void.  *data = the slot's pinned data region (slot_data_bytes).
int cec_parts_pipeline_acquire(cec_parts_pipeline* pl, size_t* slot, uint8_t** data) {
    if (!pl || !slot || !data) return CEC_ERR_INVALID_ARGUMENT;
    return pl->acquire(slot, data);
}

int cec_parts_pipeline_submit(cec_parts_pipeline* pl, size_t slot, const size_t* chunk_lens,
                              size_t n_parts) {
    if (!pl || slot >= pl->slots.size() || (n_parts && !chunk_lens) || n_parts > pl->max_parts)
        return CEC_ERR_INVALID_ARGUMENT;
    PartsSlot& s = pl->slots[slot];
    for (size_t k = 0; k < n_parts; ++k)
        if (chunk_lens[k] == 0) return CEC_EMPTY_SHARD;
    size_t data_bytes = 0, parity_bytes = 0;
    CEC_TRY(pl->place(s, chunk_lens, n_parts, &data_bytes, &parity_bytes));
    if (n_parts == 0) {  // a batch of nothing
        CEC_TRY(pl->finish(s));
        s.n_parts = 0;
        return CEC_OK;
    }
    return pl->queue_or_clear(s, chunk_lens, n_parts, data_bytes, parity_bytes, pl->whole_parts());
}

int cec_parts_pipeline_submit_from(cec_parts_pipeline* pl, size_t slot,
                                   const uint8_t* const* data_bufs, const size_t* lengths,
                                   size_t n_parts, size_t* chunksizes) {
    if (!pl || slot >= pl->slots.size() || (n_parts && (!data_bufs || !lengths || !chunksizes)) ||
        n_parts > pl->max_parts)
        return CEC_ERR_INVALID_ARGUMENT;
    PartsSlot& s = pl->slots[slot];
    for (size_t k = 0; k < n_parts; ++k)
        if (lengths[k] == 0) return CEC_EMPTY_SHARD;
    for (size_t k = 0; k < n_parts; ++k)
        if (!data_bufs[k]) return CEC_ERR_INVALID_ARGUMENT;
    std::vector<size_t> L(n_parts);
    for (size_t k = 0; k < n_parts; ++k) L[k] = (lengths[k] - 1) / pl->d + 1;
    size_t data_bytes = 0, parity_bytes = 0;
    CEC_TRY(pl->place(s, L.data(), n_parts, &data_bytes, &parity_bytes));
    CEC_TRY(pl->finish(s));  // the packing overwrites what its last batch's upload reads
    s.n_parts = 0;
    if (n_parts == 0) return CEC_OK;
    pack_parts(s.h_data, s.doffs.data(), pl->d, data_bufs, lengths, L.data(), n_parts);
    std::copy(L.begin(), L.end(), chunksizes);
    return pl->queue_or_clear(s, L.data(), n_parts, data_bytes, parity_bytes, pl->whole_parts());
}

int cec_parts_pipeline_wait(cec_parts_pipeline* pl, size_t slot, const uint8_t** parity,
                            const uint8_t** digests, size_t* n_parts) {
    return pl ? pl->wait(slot, parity, digests, n_parts) : CEC_ERR_INVALID_ARGUMENT;
}

int cec_parts_pipeline_query(cec_parts_pipeline* pl, size_t slot) {
    return pl ? pl->query(slot) : CEC_ERR_INVALID_ARGUMENT;
}

int cec_parts_pipeline_drain(cec_parts_pipeline* pl) {
    return pl ? pl->drain() : CEC_ERR_INVALID_ARGUMENT;
}

}  // extern "C"
