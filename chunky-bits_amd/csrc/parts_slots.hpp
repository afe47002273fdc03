// parts_slots.hpp — the slots of a host-staged ragged write pipeline and their steps, one copy
// each, as the parts pipeline (ragged_pipeline.cpp, which defines them) and the segment pipeline
// (segment_pipeline.cpp) share them.  Not installed, not exported.
#pragma once

#include "capi_internal.hpp"

#pragma GCC visibility push(hidden)

namespace cec {

// A slot: pinned and device regions for data, parity, digests and the launches' words, one
// non-blocking stream and one event, all made when the pipeline is made and never later.
struct PartsSlot {
    uint8_t *h_data = nullptr, *h_parity = nullptr, *h_dig = nullptr, *h_words = nullptr;  // pinned
    uint8_t *d_data = nullptr, *d_parity = nullptr, *d_dig = nullptr, *d_words = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool in_flight = false;
    size_t n_parts = 0;
    std::vector<size_t> lens, doffs, poffs;  // this batch's layout (room for max_parts)
};

// `depth` slots on one GPU and what a batch does on one of them.  A batch is a set of entries in
// the split ragged layout (cec_split_layout) over their chunk lengths.
struct PartsSlots {
    const char* who = "";  // opens the error texts
    cec_codec* codec = nullptr;
    int device = 0;
    size_t d = 0, p = 0, t = 0, data_cap = 0, parity_cap = 0, max_parts = 0;
    std::vector<PartsSlot> slots;
    size_t next = 0;

    PartsSlots() = default;
    PartsSlots(const PartsSlots&) = delete;
    PartsSlots& operator=(const PartsSlots&) = delete;
    ~PartsSlots();  // waits for every slot, frees everything, restores the caller's device

    // The size rules of a pipeline's arguments (no device use): depth 1..16, max_parts >= 1,
    // slot_data_bytes >= d * 16, sizes within size_t.  *dig = the bytes of a slot's digests.
    static int check_sizes(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts,
                           size_t depth, const char* who, size_t* dig);
    // Every allocation, on the current device: the codec's encode record, and per slot the
    // regions (words_bytes of launch words), the stream and the event.  On failure the object is
    // left for its destructor.
    int make(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts, size_t depth,
             size_t words_bytes, const char* who);

    int finish(PartsSlot& s);  // waits for the slot's batch, if one is in flight
    // The layout of a batch of these chunk lengths in the slot, and every check of it (no device
    // use).  The slot's last batch is untouched when this fails.
    int place(PartsSlot& s, const size_t* lens, size_t n, size_t* data_bytes,
              size_t* parity_bytes) const;
    // Queue the placed batch whose data lies in the slot's pinned data region: the upload,
    // launch(s) (the batch's kernels on s.stream, s.lens set), the two copies back, the event.
    using Launch = std::function<int(PartsSlot&)>;
    int queue(PartsSlot& s, const size_t* lens, size_t n, size_t data_bytes, size_t parity_bytes,
              const Launch& launch);
    // A failed queue leaves nothing of it in flight and the slot usable.
    int queue_or_clear(PartsSlot& s, const size_t* lens, size_t n, size_t data_bytes,
                       size_t parity_bytes, const Launch& launch);

    // The bodies of the C-ABI's acquire / wait / query / drain (the slot index checked here).
    int acquire(size_t* slot, uint8_t** data);
    int wait(size_t slot, const uint8_t** parity, const uint8_t** digests, size_t* n_parts);
    int query(size_t slot);
    int drain();
};

}  // namespace cec

#pragma GCC visibility pop
