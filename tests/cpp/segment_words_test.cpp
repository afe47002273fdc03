// segment_words_test.cpp — the segmented write's pure host pieces (csrc/segment_words.hpp) on the
// CPU, against their statement: the midstate record's ABI; the resume launch's and the call's word
// layouts (regions ascending, disjoint, aligned, ending at `bytes`, filled through views over heap
// buffers of exactly `bytes`); the entry rules of cec_encode_hash_segments in their order; the
// record and flags words; and the segment pipeline's open-id table over seeded random schedules:
// every column of every part goes through exactly once and in order, every refusal fires on the
// rule it names and changes nothing, and the table ends empty.
// Host code only, its own main: built plain by the library's Makefile and with
// -fsanitize=address,undefined by tests/test_segment_words.py.
#include <cstddef>
#include <cstdio>
#include <memory>
#include <random>

#include "segment_words.hpp"

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
        : bytes(bytes), h(new uint8_t[bytes]), d(new uint8_t[bytes]), v{h.get(), d.get()} {}
    template <typename T>
    void add(const plan::Region<T>& r) {
        EXPECT(r.off >= end);
        EXPECT(r.off % sizeof(T) == 0);
        EXPECT(r.end() == r.off + r.count * sizeof(T) && r.end() <= bytes);
        end = r.end();
        T *hp = v.host(r), *dp = v.dev(r);
        for (size_t i = 0; i < r.count; ++i) hp[i] = dp[i] = T(i);
    }
    size_t bytes, end = 0;
    std::unique_ptr<uint8_t[]> h, d;
    plan::View v;
};

void record_abi() {
    EXPECT(sizeof(plan::ShaMidstate) == 48 && alignof(plan::ShaMidstate) == 16);
    EXPECT(offsetof(plan::ShaMidstate, h) == 0 && offsetof(plan::ShaMidstate, bytes) == 32);
    EXPECT(offsetof(plan::ShaMidstate, reserved) == 40);
    EXPECT(plan::kMidstateBytes == 48 && plan::kSegFirst == 1u && plan::kSegLast == 2u);
}

void layouts(size_t t, size_t n) {
    const plan::SegmentWords w = plan::segment_words(t, n);
    Block b(w.bytes);
    EXPECT(w.resume.list.ptrs.off == 0);  // the upload starts at the base
    b.add(w.resume.list.ptrs);
    b.add(w.resume.list.lens);
    b.add(w.resume.list.order);
    EXPECT(w.resume.list.bytes == b.end);
    b.add(w.resume.record);
    b.add(w.resume.flags);
    EXPECT(w.resume.bytes == b.end);
    b.add(w.units);
    b.add(w.parts);
    EXPECT(b.end == w.bytes);
    const size_t items = n * t;
    EXPECT(w.resume.list.ptrs.count == items && w.resume.list.lens.count == items);
    EXPECT(w.resume.list.order.count == items && w.resume.record.count == items);
    EXPECT(w.resume.flags.count == items && w.units.count == n + 1 && w.parts.count == 6 * n);
}

void entry_rules() {
    using plan::segment_rules;
    const size_t lens[] = {64, 128, 65, 192};
    const uint32_t slots[] = {0, 1, 99, 2};
    const uint8_t F = 1, M = 0, L = 2, W = 3;
    const uint8_t ok[] = {F, M, W, L};
    EXPECT(segment_rules(lens, slots, ok, 4, 3) == 0);  // the whole part's slot is never looked at
    const uint8_t odd[] = {F, M, F, L};                 // entry 2: 65 bytes, not LAST
    EXPECT(segment_rules(lens, slots, odd, 4, 3) == 1);  // before its slot 99 is judged
    const uint8_t last_odd[] = {F, M, L, L};            // LAST may have any length; slot 99
    EXPECT(segment_rules(lens, slots, last_odd, 4, 100) == 0);
    EXPECT(segment_rules(lens, slots, last_odd, 4, 99) == 2);
    const uint32_t twice[] = {1, 1, 1, 2};
    EXPECT(segment_rules(lens, twice, ok, 4, 3) == 3);
    EXPECT(segment_rules(lens, twice, ok, 4, 1) == 2);  // the range before the duplicates
    const uint8_t whole[] = {W, W, W, W};
    EXPECT(segment_rules(lens, twice, whole, 4, 0) == 0);
    EXPECT(segment_rules(lens, slots, ok, 0, 0) == 0);

    uint32_t record[4 * 5];
    uint8_t flags[4 * 5];
    plan::resume_items(slots, ok, 4, 5, record, flags);
    for (size_t k = 0; k < 4; ++k)
        for (size_t i = 0; i < 5; ++i) {
            EXPECT(flags[k * 5 + i] == ok[k]);
            EXPECT(record[k * 5 + i] == (ok[k] == W ? 0u : slots[k] * 5 + i));
        }
}

// One part of a random schedule.
struct Part {
    size_t L, done = 0;
    uint32_t id = 0;
    bool open = false, finished = false;
};

// Random parts through an OpenIds table of max_open ids in batches of up to max_batch entries,
// segments of `seg` columns: each batch takes the next segment of every open part, then new parts
// while ids last.  Refusals are provoked on copies of valid batches.
void schedule(std::mt19937_64& rng, size_t n_parts, size_t max_open, size_t max_batch, size_t seg) {
    std::vector<Part> parts(n_parts);
    for (Part& q : parts) q.L = 1 + rng() % (max_open ? 5 * seg : seg);  // no ids: whole parts
    plan::OpenIds table(max_open);
    std::vector<uint32_t> free_ids;
    for (size_t i = max_open; i-- > 0;) free_ids.push_back(uint32_t(i));
    size_t finished = 0, next_new = 0, batches = 0;
    while (finished < n_parts) {
        std::vector<size_t> who, L, off, len;
        std::vector<uint32_t> id;
        auto add = [&](size_t q) {
            Part& x = parts[q];
            who.push_back(q);
            L.push_back(x.L);
            off.push_back(x.done);
            len.push_back(std::min(seg, x.L - x.done));
            id.push_back(x.id);
        };
        for (size_t q = 0; q < n_parts && who.size() < max_batch; ++q)
            if (parts[q].open) add(q);
        while (next_new < n_parts && who.size() < max_batch) {
            Part& x = parts[next_new];
            if (x.L > seg) {  // needs an id
                if (free_ids.empty()) break;
                x.id = free_ids.back();
                free_ids.pop_back();
            } else {
                x.id = uint32_t(rng());  // a whole part's id is never looked at
            }
            add(next_new++);
        }
        EXPECT(!who.empty());
        if (who.empty()) return;
        const size_t n = who.size();
        std::vector<uint8_t> flags(n), f2(n);
        EXPECT(table.check(L.data(), off.data(), len.data(), id.data(), n, flags.data()) == 0);
        // the refusals, each on a copy with one entry bent; nothing of the table changes
        const size_t count_before = table.count;
        for (size_t k = 0; k < n; ++k) {
            const bool whole = !plan::touches_record(flags[k]);
            auto bent = [&](std::vector<size_t> o, std::vector<size_t> l, std::vector<uint32_t> i) {
                return table.check(L.data(), o.data(), l.data(), i.data(), n, f2.data());
            };
            if (!whole) {
                auto i2 = id;
                i2[k] = uint32_t(max_open);
                EXPECT(bent(off, len, i2) == 1);
                if (flags[k] & plan::kSegFirst) {
                    for (size_t o = 0; o < max_open; ++o)
                        if (table.ids[o].open && std::find(id.begin(), id.end(), o) == id.end()) {
                            i2[k] = uint32_t(o);
                            EXPECT(bent(off, len, i2) == 3);
                            break;
                        }
                } else {
                    auto o2 = off;
                    auto l2 = len;
                    o2[k] += 64;  // skips columns
                    EXPECT(bent(o2, l2, id) == 5);
                    for (size_t o = 0; o < max_open; ++o)
                        if (!table.ids[o].open && std::find(id.begin(), id.end(), o) == id.end()) {
                            i2[k] = uint32_t(o);
                            EXPECT(bent(off, len, i2) == 4);
                            break;
                        }
                }
                for (size_t k2 = 0; k2 < n; ++k2)
                    if (k2 != k && plan::touches_record(flags[k2])) {
                        i2 = id;
                        i2[k] = id[k2];
                        EXPECT(bent(off, len, i2) == 2);
                        break;
                    }
                if (!(flags[k] & plan::kSegLast)) {
                    auto l2 = len;
                    l2[k] -= 1;  // seg is a multiple of 64, so this is not
                    EXPECT(bent(off, l2, id) == 7);
                }
            }
            if (flags[k] & plan::kSegLast) {
                auto l2 = len;
                l2[k] += 1;  // past L: no longer LAST, so a whole part now needs an id first
                const int r = bent(off, l2, id);
                EXPECT(whole ? r != 0 : r == 6);
            }
        }
        EXPECT(table.count == count_before);
        table.commit(L.data(), off.data(), len.data(), id.data(), flags.data(), n);
        ++batches;
        for (size_t k = 0; k < n; ++k) {
            Part& x = parts[who[k]];
            EXPECT(off[k] == x.done);  // in order, nothing twice
            EXPECT((off[k] == 0) == bool(flags[k] & plan::kSegFirst));
            x.done += len[k];
            EXPECT((x.done == x.L) == bool(flags[k] & plan::kSegLast));
            if (x.done == x.L) {
                x.finished = true;
                ++finished;
                if (x.open) free_ids.push_back(x.id);
                x.open = false;
            } else {
                x.open = true;
                EXPECT(table.ids[x.id].open && table.ids[x.id].done == x.done);
            }
        }
        size_t open_now = 0;
        for (const Part& x : parts) open_now += x.open;
        EXPECT(table.count == open_now && open_now <= max_open);
    }
    for (const Part& x : parts) EXPECT(x.finished && x.done == x.L);
    EXPECT(table.count == 0);
    EXPECT(!table.abandon(0));
    (void)batches;
}

void abandon() {
    plan::OpenIds table(2);
    const size_t L[] = {300}, off[] = {0}, len[] = {128};
    const uint32_t id[] = {1};
    uint8_t flags[1];
    EXPECT(table.check(L, off, len, id, 1, flags) == 0 && flags[0] == plan::kSegFirst);
    table.commit(L, off, len, id, flags, 1);
    EXPECT(table.count == 1 && !table.abandon(0) && !table.abandon(2));
    EXPECT(table.abandon(1) && table.count == 0 && !table.abandon(1));
    EXPECT(table.check(L, off, len, id, 1, flags) == 0);  // the id serves again
    const size_t off2[] = {128};
    EXPECT(table.check(L, off2, len, id, 1, flags) == 4);  // and its chain is gone
}

}  // namespace

int main() {
    record_abi();
    entry_rules();
    abandon();
    for (size_t t : {1, 5, 14})
        for (size_t n : {0, 1, 7, 61}) layouts(t, n);
    std::mt19937_64 rng(20240611);
    int runs = 0;
    for (size_t max_open : {0, 1, 3, 8})
        for (size_t seg : {64, 128, 192})
            for (int rep = 0; rep < 5; ++rep, ++runs)
                schedule(rng, 1 + rng() % 40, max_open, 1 + rng() % 12, max_open ? seg : 1u << 20);
    if (g_failed) {
        std::printf("segment_words: %d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("segment_words ok: %d random schedules\n", runs);
    return 0;
}
