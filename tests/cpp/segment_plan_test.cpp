// segment_plan_test.cpp — the batch planning of write_many_stream under many_segment
// (include/chunky_ec_segment_plan.hpp) on the CPU, over seeded random part lists, against its
// statement: every column of every part is scheduled exactly once and in order; every batch keeps
// the slot's bytes, the entry count and the open parts within their budgets and is never empty;
// a batch takes the open parts first and its entries are in part order; every batch passes the
// segment pipeline's own rules (csrc/segment_words.hpp OpenIds, the table
// cec_segment_pipeline_submit_from checks a batch against) and leaves that table empty at the
// end; and with batches collected `depth` behind their submission, the hold-back order hands the
// parts out in part order, each once, all of them.
// Host code only, its own main: built plain by the library's Makefile and with
// -fsanitize=address,undefined by tests/test_segment_plan.py.
#include <cstdio>
#include <deque>
#include <random>

#include "chunky_ec_segment_plan.hpp"
#include "segment_words.hpp"

using chunky_ec::detail::SegmentEntry;
using chunky_ec::detail::SegmentPlanner;

namespace {

int g_failed = 0;

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                               \
        }                                                             \
    } while (0)

void run(std::mt19937_64& rng, size_t d, size_t seg, size_t max_parts, size_t max_open,
         size_t depth, size_t n) {
    std::vector<size_t> L(n);
    size_t longest = 1;
    for (size_t& len : L) {
        const uint64_t r = rng();
        len = r % 4 == 0 ? 1 + (r >> 8) % (6 * seg)  // long: up to six segments
              : r % 4 == 1 ? seg * (1 + (r >> 8) % 3)  // an exact multiple
                           : 1 + (r >> 8) % seg;       // a whole part
        longest = std::max(longest, len);
    }
    const size_t entry = d * SegmentPlanner::stride16(std::min(seg, longest));
    const size_t slot = entry + (rng() % 5) * entry / 2;  // one entry, up to three
    SegmentPlanner plan(d, seg, slot, max_parts, max_open, L);
    cec::plan::OpenIds table(max_open);
    std::vector<size_t> done(n, 0), collected(n, 0);
    std::vector<bool> opened(n, false);
    std::deque<std::vector<SegmentEntry>> flying;
    size_t released = 0, batches = 0;
    auto collect = [&] {
        for (const SegmentEntry& e : flying.front()) {
            EXPECT(collected[e.part] == e.off);
            collected[e.part] += e.len;
            if (e.last) plan.complete(e.part);
            for (size_t k; (k = plan.releasable()) != SegmentPlanner::npos; plan.release()) {
                EXPECT(k == released);  // part order, each once
                EXPECT(collected[k] == L[k]);
                ++released;
            }
        }
        flying.pop_front();
    };
    while (!plan.planned()) {
        if (flying.size() == depth) collect();
        const std::vector<SegmentEntry> batch = plan.next_batch();
        ++batches;
        EXPECT(!batch.empty() && batch.size() <= max_parts);
        if (batch.empty()) return;
        size_t bytes = 0;
        bool seen_new = false;
        std::vector<size_t> bl, bo, bn;
        std::vector<uint32_t> bi;
        for (size_t q = 0; q < batch.size(); ++q) {
            const SegmentEntry& e = batch[q];
            EXPECT(q == 0 || batch[q - 1].part < e.part);  // part order
            EXPECT(e.off == done[e.part]);                 // in order, nothing twice
            EXPECT(e.len > 0 && e.len <= seg && e.off + e.len <= L[e.part]);
            EXPECT(e.first == (e.off == 0) && e.last == (e.off + e.len == L[e.part]));
            EXPECT(e.last || e.len == seg);  // only a last segment is short
            EXPECT(!(seen_new && !e.first));  // the open parts first
            seen_new = seen_new || e.first;
            if (!e.first) EXPECT(opened[e.part]);
            opened[e.part] = true;
            done[e.part] += e.len;
            bytes += d * SegmentPlanner::stride16(e.len);
            bl.push_back(L[e.part]);
            bo.push_back(e.off);
            bn.push_back(e.len);
            bi.push_back(e.id);
        }
        EXPECT(bytes <= slot);
        EXPECT(plan.open_count() <= max_open);
        // the pipeline's own view of the batch
        std::vector<uint8_t> flags(batch.size());
        EXPECT(table.check(bl.data(), bo.data(), bn.data(), bi.data(), batch.size(),
                           flags.data()) == 0);
        table.commit(bl.data(), bo.data(), bn.data(), bi.data(), flags.data(), batch.size());
        EXPECT(table.count == plan.open_count());
        // every part before the first one not yet started is under way or done: no overtaking
        flying.push_back(batch);
    }
    while (!flying.empty()) collect();
    for (size_t k = 0; k < n; ++k) EXPECT(done[k] == L[k] && collected[k] == L[k]);
    EXPECT(released == n && plan.released() == n && table.count == 0);
    EXPECT(plan.releasable() == SegmentPlanner::npos);
    size_t segments = 0;
    for (size_t len : L) segments += (len - 1) / seg + 1;
    EXPECT(batches <= segments);  // every batch carries at least one entry
}

void refusals() {
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::invalid_argument&) {
            return true;
        }
        return false;
    };
    EXPECT(throws([] { SegmentPlanner(3, 100, 4096, 8, 4, {10}); }));   // no multiple of 64
    EXPECT(throws([] { SegmentPlanner(3, 0, 4096, 8, 4, {10}); }));
    EXPECT(throws([] { SegmentPlanner(3, 128, 4096, 0, 4, {10}); }));
    EXPECT(throws([] { SegmentPlanner(3, 128, 4096, 8, 4, {10, 0}); }));
    EXPECT(throws([] { SegmentPlanner(3, 128, 4096, 8, 0, {129}); }));  // needs an id
    EXPECT(throws([] { SegmentPlanner(3, 128, 3 * 128 - 1, 8, 4, {500}); }));
    EXPECT(!throws([] { SegmentPlanner(3, 128, 3 * 128, 8, 0, {128, 1}); }));
    SegmentPlanner none(3, 128, 4096, 8, 4, {});
    EXPECT(none.planned() && none.releasable() == SegmentPlanner::npos);
}

}  // namespace

int main() {
    refusals();
    std::mt19937_64 rng(977);
    int runs = 0;
    for (size_t d : {1, 3, 10})
        for (size_t seg : {64, 128, 192})
            for (size_t max_open : {1, 2, 7})
                for (size_t depth : {1, 3})
                    for (int rep = 0; rep < 3; ++rep, ++runs)
                        run(rng, d, seg, 1 + rng() % 9, max_open, depth, rng() % 60);
    if (g_failed) {
        std::printf("segment_plan: %d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("segment_plan ok: %d random part lists\n", runs);
    return 0;
}
