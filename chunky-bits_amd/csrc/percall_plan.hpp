// percall_plan.hpp — where the per-call tier (percall.cpp) puts a batch of gathered calls, written
// as pure functions the host compiles without the HIP runtime (as plan_math.hpp / return_plan.hpp
// are): the packed ragged layout, the layout of a cec_part_encode batch (one chunk length: the
// [part][d+p][cs] block at 256-byte strides; two or more: the split layout, a data and a parity
// region) and the byte ranges a host-staged read moves up and brings back.
// tests/cpp/percall_plan_test.cpp runs them on the CPU over random batches.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace cec {

// Byte ranges [first, second) of an arena, ascending and disjoint (copy_spans' precondition).
using Spans = std::vector<std::pair<size_t, size_t>>;

// Whether a read fills slot i of a part when it is not among the verified chunks.
inline bool fills_slot(size_t i, size_t d, bool data_only) { return i < d || !data_only; }

namespace plan {

constexpr size_t kRaggedAlign = 16;  // the ragged layouts' chunk stride and offset unit
constexpr size_t kBlockAlign = 256;  // the uniform layout's chunk stride; the regions' starts

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// L rounded up to 16; 0 when that overflows.
inline size_t stride16(size_t L) {
    return L > SIZE_MAX - (kRaggedAlign - 1) ? 0 : align_up(L, kRaggedAlign);
}

// The packed ragged layout of n parts of t chunks: part k + 1 directly behind part k, chunk i of
// part k at offs[k] + i * stride16(lens[k]).  Returns 0, 1 for an empty chunk, 2 for an overflow.
inline int packed_layout(size_t t, const size_t* lens, size_t n, size_t* offs, size_t* total) {
    size_t off = 0;
    for (size_t k = 0; k < n; ++k) {
        if (lens[k] == 0) return 1;
        const size_t cs = stride16(lens[k]);
        size_t span = 0;
        if (!cs || __builtin_mul_overflow(t, cs, &span) || span > SIZE_MAX - off) return 2;
        offs[k] = off;
        off += span;
    }
    *total = off;
    return 0;
}

// ---- cec_part_encode batches ----

struct PartIn {
    size_t L;         // chunk length (nonzero)
    bool in_pinned;   // the caller's data is page-locked: moved up from where it is
    bool out_pinned;  // the caller's parity buffer is page-locked: brought back into it
};

// One request's places.  Staging offsets are into the pinned input / output staging and are
// reserved only for what is staged; device offsets are from the start of the device buffer.
struct PartPlace {
    size_t in_off;      // d rows in the input staging (in_pinned: none reserved)
    size_t out_off;     // p rows in the output staging (out_pinned: none reserved)
    size_t dev_data;    // d rows on the device
    size_t dev_parity;  // p rows on the device
    size_t dig_off;     // (d+p)*32 bytes in the digest block (device and output staging alike)
    size_t stride;      // the row stride of all four
};

struct PartTotals {
    bool mixed;        // two or more distinct chunk lengths: the split layout
    size_t in_bytes;   // input staging
    size_t out_bytes;  // parity in the output staging; the digest block lies behind it
    size_t dig_bytes;  // B * (d+p) * 32
    size_t dev_data;   // device offset of the batch's data (mixed: the data region)
    size_t dev_parity; // mixed: device offset of the parity region
    size_t dev_bytes;  // the whole device reservation: digest block first, then the chunks
};

// The layout of a batch of B requests (B > 0; lengths real buffers hold, so nothing overflows).
// One chunk length: part k's d+p rows at dev_data + k * (d+p) * cs, cs = L rounded up to 256, the
// staged ones' rows at the same stride.  Otherwise the split layout (cec_split_layout over the
// batch's L_k): rows at stride16(L_k), every part's data in one region and its parity in another,
// both behind the digest block; with no page-locked buffer in the batch the staging offsets equal
// the regions' own, so each region moves in one copy.
inline void part_layout(size_t d, size_t p, const PartIn* in, size_t B, PartPlace* out,
                        PartTotals* tot) {
    const size_t t = d + p;
    bool mixed = false;
    for (size_t k = 1; k < B; ++k) mixed = mixed || in[k].L != in[0].L;
    size_t in_bytes = 0, out_bytes = 0, data = 0, parity = 0;
    for (size_t k = 0; k < B; ++k) {
        const size_t cs = mixed ? stride16(in[k].L) : align_up(in[k].L, kBlockAlign);
        out[k].stride = cs;
        out[k].in_off = in_bytes;
        out[k].out_off = out_bytes;
        out[k].dig_off = k * t * 32;
        if (!in[k].in_pinned) in_bytes += d * cs;
        if (!in[k].out_pinned) out_bytes += p * cs;
        if (mixed) {
            out[k].dev_data = data;      // region offsets for now
            out[k].dev_parity = parity;
            data += d * cs;
            parity += p * cs;
        } else {
            out[k].dev_data = k * t * cs;
            out[k].dev_parity = k * t * cs + d * cs;
            data += t * cs;
        }
    }
    tot->mixed = mixed;
    tot->in_bytes = in_bytes;
    tot->out_bytes = out_bytes;
    tot->dig_bytes = B * t * 32;
    tot->dev_data = align_up(tot->dig_bytes, kBlockAlign);
    tot->dev_parity = mixed ? tot->dev_data + align_up(data, kBlockAlign) : 0;
    tot->dev_bytes = mixed ? tot->dev_parity + parity : tot->dev_data + data;
    for (size_t k = 0; k < B; ++k) {
        out[k].dev_data += tot->dev_data;
        out[k].dev_parity += mixed ? tot->dev_parity : tot->dev_data;
    }
}

// ---- host-staged reads (cec_parts_read, cec_part_read) ----

// The chunk slots (k, i) of a packed layout that pass pick(k, i), as byte ranges of exactly L_k
// bytes in part and chunk order: ascending and disjoint.  Returns their bytes.
template <typename Pick>
size_t chunk_spans(size_t t, const size_t* lens, const size_t* offs, size_t n, Pick pick,
                   Spans* spans) {
    size_t bytes = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t L = lens[k], cs = stride16(L);
        for (size_t i = 0; i < t; ++i)
            if (pick(k, i)) {
                spans->emplace_back(offs[k] + i * cs, offs[k] + i * cs + L);
                bytes += L;
            }
    }
    return bytes;
}

// What goes up: every loaded chunk (present[k * t + i] != 0).
inline size_t loaded_spans(size_t t, const size_t* lens, const size_t* offs, size_t n,
                           const uint8_t* present, Spans* spans) {
    return chunk_spans(t, lens, offs, n,
                       [&](size_t k, size_t i) { return present[k * t + i] != 0; }, spans);
}

// What a decodable part can return.  A part decodes once d of its chunks verify, so one with
// `loaded` chunks loaded can have slot i filled when the slot is not loaded itself, d or more are,
// and the mode fills the slot.
inline size_t loaded_count(const uint8_t* present, size_t t) {
    size_t loaded = 0;
    for (size_t i = 0; i < t; ++i) loaded += present[i] ? 1 : 0;
    return loaded;
}
inline bool may_fill(size_t i, size_t d, size_t loaded, bool data_only) {
    return loaded >= d && fills_slot(i, d, data_only);
}

// The bytes of a packed return (a stride per rebuilt chunk) if every loaded chunk verifies: what a
// reader fetches before it knows the flags.
inline size_t return_guess(size_t d, size_t t, const size_t* lens, size_t n,
                           const uint8_t* present, bool data_only) {
    size_t bytes = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t loaded = loaded_count(present + k * t, t);
        for (size_t i = 0; i < t; ++i)
            if (!present[k * t + i] && may_fill(i, d, loaded, data_only)) bytes += stride16(lens[k]);
    }
    return bytes;
}

// Whether the rebuild wrote slot i of a part: the part decoded (status 0), the chunk did not
// verify, and the mode fills the slot.
inline bool rebuilt_slot(size_t i, size_t d, bool data_only, uint8_t verified, int part_status) {
    return part_status == 0 && !verified && fills_slot(i, d, data_only);
}

// What comes back: every rebuilt chunk.
inline size_t rebuilt_spans(size_t d, size_t t, const size_t* lens, const size_t* offs, size_t n,
                            const uint8_t* verified, const int* part_status, bool data_only,
                            Spans* spans) {
    return chunk_spans(
        t, lens, offs, n,
        [&](size_t k, size_t i) {
            return rebuilt_slot(i, d, data_only, verified[k * t + i], part_status[k]);
        },
        spans);
}

}  // namespace plan
}  // namespace cec
