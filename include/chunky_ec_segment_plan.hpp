// chunky_ec_segment_plan.hpp - the batch planning of FileWriteBuilder::write_many_stream over a
// segment pipeline (many_segment): which column segments form the next batch, the slot budget, the
// allocation of open ids and the order in which finished parts may go to the store.  Pure host
// code without the C-ABI or a GPU: chunky_ec.hpp includes it, tests/cpp/segment_plan_test.cpp
// checks it on the CPU.
#ifndef CHUNKY_EC_SEGMENT_PLAN_HPP
#define CHUNKY_EC_SEGMENT_PLAN_HPP

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

namespace chunky_ec {
namespace detail {

// One entry of a batch: columns [off, off + len) of every chunk of part `part`.
struct SegmentEntry {
    size_t part, off, len;
    uint32_t id;  // the part's open id (unused by a whole part)
    bool first, last;
};

// Plans the batches of a list of parts of chunk lengths L[0 .. n), in part order, and keeps the
// order towards the store.
//   d          data chunks per part: an entry of `len` columns takes d * stride16(len) slot bytes
//   segment    columns per segment (a multiple of 64): a part with L > segment goes as
//              ceil(L / segment) entries, one per batch, holding an open id from first to last
//   slot_bytes a batch's budget of padded data bytes (at least d * stride16(min(segment, max L)))
//   max_parts  entries a batch holds at most
//   max_open   parts under way at most (the ids 0 .. max_open - 1)
// Each batch first takes the next segment of every open part, in part order, then new parts in
// part order until the slot, max_parts or the ids are used up.  So a batch's entries are in part
// order, and every batch makes progress: its first entry always fits.
class SegmentPlanner {
   public:
    static size_t stride16(size_t len) { return (len + 15) / 16 * 16; }

    SegmentPlanner(size_t d, size_t segment, size_t slot_bytes, size_t max_parts, size_t max_open,
                   std::vector<size_t> L)
        : d_(d), seg_(segment), slot_(slot_bytes), max_parts_(max_parts), L_(std::move(L)),
          complete_(L_.size(), false) {
        if (segment == 0 || segment % 64) throw std::invalid_argument("segment: a multiple of 64");
        if (max_parts == 0) throw std::invalid_argument("max_parts must be > 0");
        for (size_t len : L_) {
            if (len == 0) throw std::invalid_argument("an empty part");
            if (len > segment && max_open == 0)
                throw std::invalid_argument("a part longer than the segment needs max_open > 0");
            if (d * stride16(len < segment ? len : segment) > slot_bytes)
                throw std::invalid_argument("slot_bytes below one entry");
        }
        for (size_t i = max_open; i-- > 0;) free_.push_back(uint32_t(i));  // id 0 goes first
    }

    // Whether every column of every part has been handed out.
    bool planned() const { return next_new_ == L_.size() && open_.empty(); }
    size_t open_count() const { return open_.size(); }

    // The next batch (never empty while !planned()).
    std::vector<SegmentEntry> next_batch() {
        std::vector<SegmentEntry> batch;
        size_t room = slot_;
        auto fits = [&](size_t len) {
            return batch.size() < max_parts_ && d_ * stride16(len) <= room;
        };
        std::vector<Open> still;
        std::vector<uint32_t> freed;  // by this batch's last entries: a batch names an id once,
                                      // so they serve other parts from the next batch on
        for (const Open& o : open_) {  // the open parts first, in part order
            const size_t len = next_len(o.part, o.done);
            if (!fits(len)) {
                still.push_back(o);
                continue;
            }
            const bool last = o.done + len == L_[o.part];
            batch.push_back({o.part, o.done, len, o.id, false, last});
            room -= d_ * stride16(len);
            if (last)
                freed.push_back(o.id);
            else
                still.push_back({o.part, o.done + len, o.id});
        }
        while (next_new_ < L_.size()) {  // then new parts, in part order
            const size_t part = next_new_, len = next_len(part, 0);
            const bool whole = len == L_[part];
            if (!fits(len) || (!whole && free_.empty())) break;
            uint32_t id = 0;
            if (!whole) {
                id = free_.back();
                free_.pop_back();
                still.push_back({part, len, id});
            }
            batch.push_back({part, 0, len, id, true, whole});
            room -= d_ * stride16(len);
            ++next_new_;
        }
        free_.insert(free_.end(), freed.begin(), freed.end());
        open_.swap(still);
        return batch;
    }

    // The hold-back order: parts go to the store in part order.  complete(part): the part's last
    // entry has been collected.  releasable(): the next part to go, or npos while that one is
    // not complete; release() moves on.
    static constexpr size_t npos = size_t(-1);
    void complete(size_t part) { complete_[part] = true; }
    size_t releasable() const {
        return cursor_ < L_.size() && complete_[cursor_] ? cursor_ : npos;
    }
    void release() { ++cursor_; }
    size_t released() const { return cursor_; }

   private:
    struct Open {
        size_t part, done;
        uint32_t id;
    };
    size_t next_len(size_t part, size_t done) const {
        const size_t left = L_[part] - done;
        return left < seg_ ? left : seg_;
    }

    size_t d_, seg_, slot_, max_parts_;
    std::vector<size_t> L_;
    std::vector<bool> complete_;
    std::vector<Open> open_;      // in part order
    std::vector<uint32_t> free_;  // free ids, the next one to give out last
    size_t next_new_ = 0, cursor_ = 0;
};

}  // namespace detail
}  // namespace chunky_ec

#endif  // CHUNKY_EC_SEGMENT_PLAN_HPP
