// scrub_words_test.cpp — the segmented scrub's pure host pieces (csrc/scrub_words.hpp) on the CPU,
// against their statement: the word layout of a verifying resume launch (regions ascending,
// disjoint, aligned, inside `bytes`, the expected rows 16-byte aligned and the end of what goes up,
// the ok bytes behind it; filled through views over heap buffers of exactly `bytes`); the record
// indices of a list with one chunk per part; the filled list (addresses, lengths, longest first);
// and the call's rule table over seeded random entry lists, against a restatement written here.
// Host code only, its own main: built plain by the library's Makefile and with
// -fsanitize=address,undefined by tests/test_scrub_words.py.
#include <cstddef>
#include <cstdio>
#include <memory>
#include <random>
#include <set>

#include "scrub_words.hpp"

using namespace cec;

namespace {

int g_failed = 0;

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                               \
        }                                                             \
    } while (0)

struct Block {
    explicit Block(size_t bytes)
        : bytes(bytes), h(new uint8_t[bytes + 1]), d(new uint8_t[bytes + 1]), v{h.get(), d.get()} {}
    template <typename T>
    void add(const plan::Region<T>& r) {
        EXPECT(r.off >= end);
        EXPECT(r.off % alignof(T) == 0);
        EXPECT(r.end() == r.off + r.count * sizeof(T) && r.end() <= bytes);
        end = r.end();
        uint8_t *hp = reinterpret_cast<uint8_t*>(v.host(r)), *dp = reinterpret_cast<uint8_t*>(v.dev(r));
        for (size_t i = 0; i < r.count * sizeof(T); ++i) hp[i] = dp[i] = uint8_t(i);
    }
    size_t bytes, end = 0;
    std::unique_ptr<uint8_t[]> h, d;
    plan::View v;
};

void layout(size_t n) {
    const plan::ScrubWords w = plan::scrub_words(n);
    Block b(w.bytes);
    EXPECT(w.resume.list.ptrs.off == 0);  // the upload starts at the base
    b.add(w.resume.list.ptrs);
    b.add(w.resume.list.lens);
    b.add(w.resume.list.order);
    b.add(w.resume.record);
    b.add(w.resume.flags);
    EXPECT(w.resume.bytes == b.end);  // a caller with device rows sends this much
    b.add(w.expected);
    EXPECT(w.expected.off % 16 == 0);  // the kernel reads a row as two 16-byte vectors
    EXPECT(w.up_bytes == b.end);       // the pipeline's upload ends with the rows
    b.add(w.ok);
    EXPECT(w.ok.off >= w.up_bytes);  // only comes back
    EXPECT(b.end == w.bytes);
    EXPECT(w.resume.list.ptrs.count == n && w.resume.list.lens.count == n);
    EXPECT(w.resume.list.order.count == n && w.resume.record.count == n);
    EXPECT(w.resume.flags.count == n && w.expected.count == n && w.ok.count == n);
    // the same list the segmented write has with one chunk per part
    plan::Cursor c;
    const plan::ResumeWords r = plan::resume_words(c, n);
    EXPECT(r.bytes == w.resume.bytes && r.record.off == w.resume.record.off);
    if (n) EXPECT(plan::scrub_words(n - 1).bytes <= w.bytes);  // a slot sized for n holds fewer
}

// The rule table restated: the first rule broken, rule by rule over the whole call.
int rules_restated(const std::vector<size_t>& lens, const std::vector<uint32_t>& slots,
                   const std::vector<uint8_t>& flags, size_t n_slots) {
    const size_t n = lens.size();
    auto touches = [&](size_t k) { return (flags[k] & 3) != 3; };
    for (size_t k = 0; k < n; ++k)
        if (!(flags[k] & 2) && lens[k] % 64) return 1;
    for (size_t k = 0; k < n; ++k)
        if (touches(k) && slots[k] >= n_slots) return 2;
    std::set<uint32_t> seen;
    for (size_t k = 0; k < n; ++k)
        if (touches(k) && !seen.insert(slots[k]).second) return 3;
    return 0;
}

void random_entries(std::mt19937_64& rng, int* seen_rule) {
    const size_t n = rng() % 12, n_slots = rng() % 10;
    std::vector<size_t> lens(n), offs(n);
    std::vector<uint32_t> slots(n);
    std::vector<uint8_t> flags(n);
    size_t at = 0;
    for (size_t k = 0; k < n; ++k) {
        flags[k] = uint8_t(rng() % 4);
        const bool last = flags[k] & 2;
        lens[k] = !last && rng() % 8 ? 64 * (1 + rng() % 5) : 1 + rng() % 400;
        const uint64_t kind = rng(), pick = rng();  // one draw per statement: the same everywhere
        slots[k] = uint32_t(kind % 8 ? pick % (n_slots + (kind % 6 == 0) + 1) : 0xFFFFFFFFu);
        offs[k] = at;
        at += plan::stride16(lens[k]) + 16 * (rng() % 3);
    }
    const int want = rules_restated(lens, slots, flags, n_slots);
    const int got = plan::scrub_rules(lens.data(), slots.data(), flags.data(), n, n_slots);
    EXPECT(got == want);
    ++seen_rule[want];
    bool whole = true;
    for (size_t k = 0; k < n; ++k) whole = whole && (flags[k] & 3) == 3;
    EXPECT(plan::all_whole(flags.data(), n) == whole);
    if (want != 0) return;
    // a sound call: the filled words
    const plan::ScrubWords w = plan::scrub_words(n);
    Block b(w.bytes);
    const uint64_t base = 0x7000000000ull;
    plan::scrub_fill(base, offs.data(), lens.data(), n, slots.data(), flags.data(), w.resume, b.v);
    const uint64_t* ptrs = b.v.host(w.resume.list.ptrs);
    const uint64_t* hl = b.v.host(w.resume.list.lens);
    const uint32_t* order = b.v.host(w.resume.list.order);
    const uint32_t* record = b.v.host(w.resume.record);
    const uint8_t* fl = b.v.host(w.resume.flags);
    std::set<uint32_t> listed;
    for (size_t k = 0; k < n; ++k) {
        EXPECT(ptrs[k] == base + offs[k] && hl[k] == lens[k]);
        EXPECT(fl[k] == flags[k]);
        // record indices with one chunk per part: the slot itself, 0 for a whole entry
        EXPECT(record[k] == ((flags[k] & 3) == 3 ? 0u : slots[k]));
        EXPECT(order[k] < n && listed.insert(order[k]).second);
        if (k) EXPECT(lens[order[k - 1]] >= lens[order[k]]);  // longest first
    }
}

}  // namespace

int main() {
    for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(3), size_t(7), size_t(64), size_t(257),
                     size_t(4096)})
        layout(n);
    std::mt19937_64 rng(20250607);
    int seen_rule[4] = {0, 0, 0, 0};
    const int lists = 4000;
    for (int i = 0; i < lists; ++i) random_entries(rng, seen_rule);
    for (int r = 0; r < 4; ++r) EXPECT(seen_rule[r] > 20);  // every rule is reached
    if (g_failed) {
        std::printf("scrub_words FAILED: %d checks\n", g_failed);
        return 1;
    }
    std::printf("scrub_words ok: %d random entry lists (rules 0..3 hit %d %d %d %d times)\n", lists,
                seen_rule[0], seen_rule[1], seen_rule[2], seen_rule[3]);
    return 0;
}
