// scrub_words.hpp — the segmented scrub (cec_verify_segments, scrub_pipeline.cpp): where the words
// of the verifying resume launch (sha256_resume_kernels.hip sha256_resume_verify_kernel) lie in
// their buffer, and the pure host functions that check a call's entries and fill those words,
// written so that the host compiles them without the HIP runtime (as segment_words.hpp is, whose
// record, rules and open-id table they use as they are: to the scrub a copy is a part of one
// chunk, d = 1, t = 1, of chunk length = its length).
#pragma once

#include "segment_words.hpp"

namespace cec {
namespace plan {

// One expected digest, as the kernel reads it: two 16-byte vectors.
struct alignas(16) DigestRow {
    uint8_t b[32];
};
static_assert(sizeof(DigestRow) == 32, "a SHA-256 digest");

// A segmented verification of n entries: [the resume list of n items][expected 32 B x n][ok u8 x n].
// The list and the expected rows go up in one copy of `up_bytes` (a caller whose expected rows are
// on the device already sends the list alone, resume.bytes); the ok bytes, which only come back,
// lie behind what goes up.
struct ScrubWords {
    ResumeWords resume;
    Region<DigestRow> expected;
    size_t up_bytes;
    Region<uint8_t> ok;
    size_t bytes;
};
inline ScrubWords scrub_words(size_t n) {
    Cursor c;
    return {resume_words(c, n), c.take<DigestRow>(n), c.at, c.take<uint8_t>(n), c.at};
}

// The entry rules of cec_verify_segments behind the layout's own: segment_rules' table (0 = fine,
// 1 = a non-LAST length that is no multiple of 64, 2 = a slot >= n_slots, 3 = a slot named by two
// record-touching entries).
inline int scrub_rules(const size_t* seg_lens, const uint32_t* slots, const uint8_t* flags,
                       size_t n, size_t n_slots) {
    return segment_rules(seg_lens, slots, flags, n, n_slots);
}

// Whether no entry of a call touches a record (the pool may then be null).
inline bool all_whole(const uint8_t* flags, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (touches_record(flags[k])) return false;
    return true;
}

// The resume list of n checked entries, entry k = seg_lens[k] bytes at address base + offs[k]:
// ptrs, lens and order (longest first, sha_list with one chunk per part), and the record and flags
// words (resume_items with t = 1: item k uses record slots[k]).
inline void scrub_fill(uint64_t base, const size_t* offs, const size_t* seg_lens, size_t n,
                       const uint32_t* slots, const uint8_t* flags, const ResumeWords& w,
                       const View& v) {
    sha_list(
        seg_lens, n, 1, [](size_t) { return true; },
        [&](size_t k, size_t, size_t) { return base + offs[k]; }, v.host(w.list.ptrs),
        v.host(w.list.lens), v.host(w.list.order));
    resume_items(slots, flags, n, 1, v.host(w.record), v.host(w.flags));
}

}  // namespace plan
}  // namespace cec
