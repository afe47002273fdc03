// ragged_words.hpp — where the words of the ragged tier's launches (ragged.cpp) lie in their
// scratch buffers, and the pure host functions that fill them, written so that the host compiles
// them without the HIP runtime (as percall_plan.hpp is).  A layout is a struct of typed regions
// plus `bytes`, made by one function; a View hands out a region's pointer on the page-locked and
// on the device side.  tests/cpp/ragged_words_test.cpp checks all of it on the CPU.
#pragma once

#include <algorithm>
#include <numeric>

#include "percall_plan.hpp"

namespace cec {
namespace plan {

// `count` elements of T at byte offset `off` of a words buffer.
template <typename T>
struct Region {
    size_t off = 0, count = 0;
    size_t end() const { return off + count * sizeof(T); }
};

// Hands out a layout's regions one behind the other, each aligned to its element.  The layouts
// below take them inside braces, whose elements the language evaluates from left to right: the
// regions lie in the order they are written, and the closing c.at is the end of the last one.
struct Cursor {
    size_t at = 0;
    template <typename T>
    Region<T> take(size_t count) {
        const Region<T> r{align_up(at, sizeof(T)), count};
        at = r.end();
        return r;
    }
};

// A words buffer's two sides (either may be null: never asked for).
struct View {
    uint8_t *h, *d;
    template <typename T>
    T* host(const Region<T>& r) const { return reinterpret_cast<T*>(h + r.off); }
    template <typename T>
    T* dev(const Region<T>& r) const { return reinterpret_cast<T*>(d + r.off); }
};

// The SHA-256 list of `items` chunks: [ptrs u64 x items][lens u64 x items][order u32 x items].
// `bytes` is also where a caller's own words (its "tail") begin, which go up in the list's copy.
struct ShaListWords {
    Region<uint64_t> ptrs, lens;
    Region<uint32_t> order;
    size_t bytes;
    // what goes up when there is no tail: the list as far as the `hashed` listed items reach
    size_t up_bytes(size_t hashed) const { return hashed ? order.off + hashed * 4 : 0; }
};
inline ShaListWords sha_list_words(Cursor& c, size_t items) {
    return {c.take<uint64_t>(items), c.take<uint64_t>(items), c.take<uint32_t>(items), c.at};
}

// A ragged encode of n parts of t chunks.  Two-pass: [the SHA-256 list][units u32 x n+1]
// [parts u32 x 4n, split: 6n]; fused: [order u32 x n][parts], the part order where the SHA-256
// list would be, which is less.
struct EncodeWords {
    ShaListWords list;
    Region<uint32_t> units, parts;
    size_t bytes;
};
inline EncodeWords encode_words(size_t t, size_t n, bool fused, bool split) {
    Cursor c;
    const size_t w = split ? 6 : 4;
    if (fused) return {{{}, {}, c.take<uint32_t>(n), c.at}, {}, c.take<uint32_t>(n * w), c.at};
    return {sha_list_words(c, n * t), c.take<uint32_t>(n + 1), c.take<uint32_t>(n * w), c.at};
}
// Bytes of words that hold any ragged encode of n parts of t chunks (a caller-owned buffer's size).
inline size_t ragged_words_bytes(size_t t, size_t n) {
    size_t bytes = 0;
    for (int v = 0; v < 4; ++v) bytes = std::max(bytes, encode_words(t, n, v & 1, v & 2).bytes);
    return bytes;
}

// A ragged verification with a readback: [the SHA-256 list][ok u8 x items].
struct VerifyWords {
    ShaListWords list;
    Region<uint8_t> ok;
    size_t bytes;
};
inline VerifyWords verify_words(size_t items) {
    Cursor c;
    return {sha_list_words(c, items), c.take<uint8_t>(items), c.at};
}

// What an async read of n parts of t chunks uploads, in one copy: [the SHA-256 list]
// [units u32 x n+1][parts u32 x 4n][part_pat u32 x n][present u8 x n*t].
struct ReadUpWords {
    ShaListWords list;
    Region<uint32_t> units, parts, part_pat;
    Region<uint8_t> present;
    size_t bytes;
};
inline ReadUpWords read_up_words(size_t t, size_t n) {
    Cursor c;
    return {sha_list_words(c, n * t), c.take<uint32_t>(n + 1), c.take<uint32_t>(n * 4),
            c.take<uint32_t>(n),      c.take<uint8_t>(n * t),  c.at};
}

// What stays on the device: [records u32 x n*slot][status i32 x n][ok u8 x n*t][verified u8 x n*t]
// and, with a packed return, [ret_off u64 x n+1] behind them.
struct ReadDevWords {
    Region<uint32_t> records;
    Region<int32_t> status;
    Region<uint8_t> ok, verified;
    Region<uint64_t> ret_off;
    size_t bytes;
};
inline ReadDevWords read_dev_words(size_t t, size_t n, size_t slot, bool packed) {
    Cursor c;
    return {c.take<uint32_t>(n * slot), c.take<int32_t>(n), c.take<uint8_t>(n * t),
            c.take<uint8_t>(n * t), packed ? c.take<uint64_t>(n + 1) : Region<uint64_t>{}, c.at};
}

// A host-planned reconstruct: [plan words][per launch: units u32 x count+1, parts u32 x 4 count].
// `launches`: anything that has a `count` of listed parts per launch (DecodePlan::launches).
struct ReconWords {
    Region<uint32_t> plan;
    std::vector<Region<uint32_t>> units, parts;  // by launch
    size_t bytes;
};
template <typename Launches>
ReconWords recon_words(size_t plan_words, const Launches& launches) {
    Cursor c;
    ReconWords w{c.take<uint32_t>(plan_words), {}, {}, 0};
    for (const auto& l : launches) {
        w.units.push_back(c.take<uint32_t>(l.count + 1));
        w.parts.push_back(c.take<uint32_t>(4 * l.count));
    }
    w.bytes = c.at;
    return w;
}

// The per-part device records of the parts ids[0 .. count) (null: parts 0 .. count - 1):
// units[count + 1] = the prefix array of their work units of `unit` bytes (null: not wanted),
// parts[4 * count] = {off lo, off hi, L lo, L hi}.  Returns the unit total.
// With `disp` (the split layout, kernels.hpp RaggedParams::split) a record has two more words,
// {disp lo, disp hi}: parts[6 * count].
inline uint32_t part_records(uint64_t unit, const size_t* offs, const size_t* lens,
                             const uint32_t* ids, size_t count, uint32_t* units, uint32_t* parts,
                             const uint64_t* disp = nullptr) {
    auto put = [&](uint64_t x) {  // the next two words: lo, hi
        *parts++ = uint32_t(x);
        *parts++ = uint32_t(x >> 32);
    };
    uint64_t acc = 0;
    for (size_t q = 0; q < count; ++q) {
        const size_t k = ids ? ids[q] : q;
        if (units) units[q] = uint32_t(acc);
        acc += (uint64_t(lens[k]) - 1) / unit + 1;
        put(offs[k]);
        put(lens[k]);
        if (disp) put(disp[k]);
    }
    if (units) units[count] = uint32_t(acc);
    return uint32_t(acc);
}

// order[n] = the parts stably sorted by chunk length, longest first.
inline void length_order(const size_t* lens, size_t n, uint32_t* order) {
    std::iota(order, order + n, 0u);
    std::stable_sort(order, order + n, [&](uint32_t x, uint32_t y) { return lens[x] > lens[y]; });
}

// The SHA-256 list of a ragged batch: ptrs / h_len of the items k * t + i that pass `pick` (the
// others are never looked at) and, in `order`, those items stably sorted by their part's length,
// longest first: a SHA-256 wave runs as long as its longest lane, so the 64 chains of a wave get
// similar lengths.  Digests and flags land at their item's place whatever the order.  An item's
// key is its part's, so the parts are sorted and each expanded in place.  Returns the items listed.
// at(k, i, stride) is where part k's chunk i lies (a pointer or an address).
template <typename Pick, typename At>
size_t sha_list(const size_t* lens, size_t n, size_t t, Pick pick, At at, uint64_t* ptrs,
                uint64_t* h_len, uint32_t* order) {
    std::vector<uint32_t> by_len(n);
    length_order(lens, n, by_len.data());
    size_t count = 0;
    for (const size_t k : by_len) {
        const size_t cs = stride16(lens[k]);
        for (size_t i = 0; i < t; ++i) {
            const size_t item = k * t + i;
            if (!pick(item)) continue;
            ptrs[item] = (uint64_t)at(k, i, cs);
            h_len[item] = lens[k];
            order[count++] = uint32_t(item);
        }
    }
    return count;
}

}  // namespace plan
}  // namespace cec
