// segment_words.hpp — the segmented ragged write (cec_encode_hash_segments, segment_pipeline.cpp):
// the SHA-256 midstate record that carries a chunk's chain from one launch to the next, where the
// words of the resume launch (sha256_resume_kernels.hip) lie in their buffer, and the pure host
// functions that check a call's entries and fill those words, written so that the host compiles
// them without the HIP runtime (as ragged_words.hpp is).
#pragma once

#include <vector>

#include "ragged_words.hpp"

namespace cec {
namespace plan {

// The state of one chunk's chain after a whole number of 64-byte blocks: FIPS 180-4's eight
// working words and the bytes hashed so far.  48 bytes, 16-byte aligned; the kernel reads and
// writes it as three 16-byte vectors.
struct alignas(16) ShaMidstate {
    uint32_t h[8];
    uint64_t bytes;
    uint64_t reserved;
};
static_assert(sizeof(ShaMidstate) == 48 && alignof(ShaMidstate) == 16, "the ABI's 48-byte record");
constexpr size_t kMidstateBytes = sizeof(ShaMidstate);

// An item's flags (CEC_SEG_FIRST / CEC_SEG_LAST of the header, the same values).
constexpr uint32_t kSegFirst = 1u, kSegLast = 2u;

// The resume launch's list of `items` chunk segments: the SHA-256 list
// [ptrs u64 x items][lens u64 x items][order u32 x items] and behind it
// [record u32 x items][flags u8 x items].  record[item] = the item's midstate record (an index
// into the pool), flags[item] = kSegFirst | kSegLast bits; both indexed by item like ptrs and lens.
struct ResumeWords {
    ShaListWords list;
    Region<uint32_t> record;
    Region<uint8_t> flags;
    size_t bytes;
};
inline ResumeWords resume_words(Cursor& c, size_t items) {
    return {sha_list_words(c, items), c.take<uint32_t>(items), c.take<uint8_t>(items), c.at};
}

// A segmented encode of n entries of t chunks: [the resume list][units u32 x n+1][parts u32 x 6n]
// (the split layout's part records, ragged_words.hpp part_records).
struct SegmentWords {
    ResumeWords resume;
    Region<uint32_t> units, parts;
    size_t bytes;
};
inline SegmentWords segment_words(size_t t, size_t n) {
    Cursor c;
    return {resume_words(c, n * t), c.take<uint32_t>(n + 1), c.take<uint32_t>(n * 6), c.at};
}

// Whether an entry reads or writes its slot's records: everything but a whole part.
inline bool touches_record(uint8_t flags) {
    return (flags & (kSegFirst | kSegLast)) != (kSegFirst | kSegLast);
}

// The segment rules of a call's entries behind the layout's own: 0 = fine, 1 = a non-LAST length
// that is no multiple of 64, 2 = a slot >= n_slots, 3 = a slot named by two record-touching
// entries.  In this order over the whole call: every length, then every slot's range, then the
// duplicates.  Entries that are FIRST|LAST touch no record and their slot is never looked at.
inline int segment_rules(const size_t* seg_lens, const uint32_t* slots, const uint8_t* flags,
                         size_t n, size_t n_slots) {
    for (size_t k = 0; k < n; ++k)
        if (!(flags[k] & kSegLast) && seg_lens[k] % 64) return 1;
    for (size_t k = 0; k < n; ++k)
        if (touches_record(flags[k]) && slots[k] >= n_slots) return 2;
    std::vector<uint32_t> used;
    for (size_t k = 0; k < n; ++k)
        if (touches_record(flags[k])) used.push_back(slots[k]);
    std::sort(used.begin(), used.end());
    return std::adjacent_find(used.begin(), used.end()) != used.end() ? 3 : 0;
}

// The resume list's record and flags words of n entries of t chunks: item k * t + i uses record
// slots[k] * t + i (0 for an entry that touches none) and its entry's flags.
inline void resume_items(const uint32_t* slots, const uint8_t* flags, size_t n, size_t t,
                         uint32_t* record, uint8_t* item_flags) {
    for (size_t k = 0; k < n; ++k)
        for (size_t i = 0; i < t; ++i) {
            record[k * t + i] = touches_record(flags[k]) ? uint32_t(slots[k] * t + i) : 0u;
            item_flags[k * t + i] = flags[k] & uint8_t(kSegFirst | kSegLast);
        }
}

// The open ids of a segment pipeline: which parts are under way, their chunk length and the
// columns submitted so far.  A batch is checked as a whole (nothing changes), then committed.
struct OpenIds {
    struct Id {
        bool open = false;
        size_t L = 0, done = 0;
    };
    std::vector<Id> ids;
    size_t count = 0;

    explicit OpenIds(size_t max_open = 0) : ids(max_open) {}

    // The flags of an entry: FIRST when its range starts at column 0, LAST when it ends at L.
    static uint8_t entry_flags(size_t L, size_t off, size_t len) {
        return uint8_t((off == 0 ? kSegFirst : 0u) | (len <= L && off == L - len ? kSegLast : 0u));
    }

    // The rules of a batch of n entries (chunk lengths L, column ranges [offs, offs + lens), ids),
    // rule by rule over the whole batch: 0 = fine, else the first rule broken:
    //   1 an id >= max_open                 2 an id twice in the batch
    //   3 a FIRST (not LAST) on an open id  4 a continuation on an id that is not open
    //   5 a continuation whose offset is not the columns so far, or whose L changed
    //   6 a range past L                    7 a length without LAST that is no multiple of 64
    // Whole parts (FIRST | LAST) have no id: theirs is never looked at.  flags[n] is written.
    int check(const size_t* L, const size_t* offs, const size_t* lens, const uint32_t* id, size_t n,
              uint8_t* flags) const {
        for (size_t k = 0; k < n; ++k) flags[k] = entry_flags(L[k], offs[k], lens[k]);
        auto each = [&](auto broken) {  // over the entries that have an id
            for (size_t k = 0; k < n; ++k)
                if (touches_record(flags[k]) && broken(k)) return true;
            return false;
        };
        if (each([&](size_t k) { return id[k] >= ids.size(); })) return 1;
        std::vector<uint32_t> used;
        each([&](size_t k) { return used.push_back(id[k]), false; });
        std::sort(used.begin(), used.end());
        if (std::adjacent_find(used.begin(), used.end()) != used.end()) return 2;
        if (each([&](size_t k) { return (flags[k] & kSegFirst) && ids[id[k]].open; })) return 3;
        if (each([&](size_t k) { return !(flags[k] & kSegFirst) && !ids[id[k]].open; })) return 4;
        if (each([&](size_t k) {
                const Id& o = ids[id[k]];
                return !(flags[k] & kSegFirst) && (offs[k] != o.done || L[k] != o.L);
            }))
            return 5;
        for (size_t k = 0; k < n; ++k)
            if (offs[k] > L[k] || lens[k] > L[k] - offs[k]) return 6;
        for (size_t k = 0; k < n; ++k)
            if (!(flags[k] & kSegLast) && lens[k] % 64) return 7;
        return 0;
    }

    // The checked batch was queued: a FIRST opens its id, a LAST closes it, the others move on.
    void commit(const size_t* L, const size_t* offs, const size_t* lens, const uint32_t* id,
                const uint8_t* flags, size_t n) {
        for (size_t k = 0; k < n; ++k) {
            if (!touches_record(flags[k])) continue;
            Id& o = ids[id[k]];
            if (flags[k] & kSegFirst) ++count;
            if (flags[k] & kSegLast) --count;
            o = Id{!(flags[k] & kSegLast), L[k], offs[k] + lens[k]};
        }
    }

    // Closes an open id; false if it is not open.
    bool abandon(size_t i) {
        if (i >= ids.size() || !ids[i].open) return false;
        ids[i] = Id{};
        --count;
        return true;
    }
};

}  // namespace plan
}  // namespace cec
