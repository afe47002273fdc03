// verify_many_stream_host_fuzz.cpp — FileReference::verify_many_stream's host loop
// (include/chunky_ec.hpp: the copy list under the skeleton rule, the batches of
// detail::SegmentPlanner, the expected rows, the collection of verdicts and the summaries) on the
// CPU, with cec_scrub_pipeline_* replaced by stand-ins that enforce the contract of
// include/chunky_ec_scrub.h and compute with the oracle (test infrastructure: this binary is built
// and run only by tests/test_cpp_verify_many_stream_host.py, plain and under ASan + UBSan).
//
// The stand-ins count what the header promises the engine and the caller breaks: a batch that
// csrc/segment_words.hpp's OpenIds table refuses (an id out of range, twice in a batch, reused
// before its LAST, a continuation that is out of order, a range past the copy, a length that is
// no multiple of 64), a batch beyond the slot's capacity or entry count, a slot submitted without
// being acquired, a null or empty copy.  They read an expected row only for an entry that ends its
// copy (every other row is poisoned by the program's own check below: the loop sends zeros there,
// and a verdict that depended on one would differ), hash the bytes accumulated per open id with
// or_sha256, and hand the verdicts out only in wait: until then, and from the next acquire on, the
// slot's flags hold a poison value, so results read too early or too late give wrong reports.
//
// Each seed: check_many_host_fuzz.cpp's files (a few files of random sizes and shapes RS(3,2),
// RS(10,4), RS(2,10), chunks of 16 to 512 bytes, every chunk stored with a random mix of
// locations: good; [bad, good]; [good, bad]; [gone, short, good]; [good, good]; [bad, bad]; bad;
// short; gone).  Checked: verify_many_stream equals verify() file by file for several segment and
// slot sizes, a slot of one segment and max_open = 1 among them, and no id stays open.
// Usage: verify_many_stream_host_fuzz FIRST_SEED N_SEEDS; exit status 0 iff every seed passed.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "chunky_ec.hpp"
#include "segment_words.hpp"  // csrc: the open-id table the engine itself uses

extern "C" {
// oracle/cec_oracle.c
void or_sha256(const uint8_t* buf, size_t len, uint8_t out[32]);
int or_rs_encode_sep(size_t d, size_t p, const uint8_t* const* data, const size_t* data_lens,
                     size_t n_data, uint8_t* const* parity, const size_t* parity_lens,
                     size_t n_parity);
}

namespace {

int g_violations = 0;  // contract breaches seen by the stand-ins
size_t g_batches = 0, g_entries = 0, g_continued = 0, g_whole = 0, g_one_open = 0, g_reused = 0;

void violation(const char* what) {
    std::fprintf(stderr, "  contract: %s\n", what);
    ++g_violations;
}

constexpr uint8_t kPoison = 0xEE;  // neither 0 nor 1: "not yours to read"

}  // namespace

struct cec_codec {
    size_t d, p;
};

// The stand-in pipeline: the engine's own open-id table, the bytes of every open copy so far, and
// per slot the verdicts, visible from wait to the next acquire.
struct cec_scrub_pipeline {
    size_t slot_bytes, max_entries;
    cec::plan::OpenIds open;
    std::vector<std::vector<uint8_t>> so_far;  // per id
    std::vector<bool> id_used;                 // ids that have served a copy before
    struct Slot {
        bool acquired = false, in_flight = false;
        std::vector<uint8_t> hidden, shown;  // the batch's verdicts; what the caller may read
    };
    std::vector<Slot> slots;
    size_t next = 0;
};

namespace {
cec_scrub_pipeline* g_pipeline = nullptr;  // the one in use (the header caches one per thread)
}

extern "C" {

const char* cec_status_name(int) { return "status"; }
const char* cec_last_error(void) { return ""; }
int cec_codec_new(size_t d, size_t p, cec_codec** out) {
    if (!d || !p || d + p > 256) return CEC_TOO_MANY_SHARDS;
    *out = new cec_codec{d, p};
    return CEC_OK;
}
void cec_codec_free(cec_codec* c) { delete c; }
size_t cec_codec_data_shards(const cec_codec* c) { return c->d; }
size_t cec_codec_parity_shards(const cec_codec* c) { return c->p; }
size_t cec_codec_total_shards(const cec_codec* c) { return c->d + c->p; }

// verify() with parts_per_batch = 0 hashes through check_locations.  Called from several threads.
int cec_sha256_many(const uint8_t* const* bufs, const size_t* lens, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; ++i) or_sha256(bufs[i], lens[i], out + 32 * i);
    return CEC_OK;
}

// Nothing here rebuilds, batches through the scheduler or takes the one-call path.
static int unreached(const char* what) {
    violation(what);
    return CEC_ERR_INVALID_ARGUMENT;
}
int cec_reconstruct(const cec_codec*, uint8_t* const*, const size_t*, uint8_t*, size_t) {
    return unreached("cec_reconstruct called");
}
int cec_reconstruct_data(const cec_codec*, uint8_t* const*, const size_t*, uint8_t*, size_t) {
    return unreached("cec_reconstruct_data called");
}
int cec_host_alloc(size_t, int, void**) { return unreached("cec_host_alloc called"); }
void cec_host_free(void*) { unreached("cec_host_free called"); }
int cec_multi_new(const cec_codec*, size_t, size_t, size_t, const int*, size_t, cec_multi**) {
    return unreached("cec_multi_new called");
}
void cec_multi_free(cec_multi*) { unreached("cec_multi_free called"); }
int cec_multi_verify(cec_multi*, const uint8_t*, const uint8_t*, const uint8_t*, size_t,
                     uint8_t*, uint64_t*) {
    return unreached("cec_multi_verify called");
}
int cec_multi_resilver(cec_multi*, const uint8_t*, const uint8_t*, const uint8_t*, size_t,
                       uint8_t*, uint8_t*, int*, const uint8_t**, uint64_t*) {
    return unreached("cec_multi_resilver called");
}
int cec_multi_wait(cec_multi*, uint64_t) { return unreached("cec_multi_wait called"); }
const char* cec_multi_last_error(void) { return "no scheduler here"; }
int cec_parts_verify(const uint8_t* const*, const size_t*, size_t, const uint8_t*, uint8_t*) {
    return unreached("cec_parts_verify called: the stream has its own path");
}

int cec_current_device(int* dev) {
    *dev = 0;
    return CEC_OK;
}

int cec_scrub_pipeline_new(size_t slot_bytes, size_t max_entries, size_t depth, size_t max_open,
                           cec_scrub_pipeline** out) {
    if (!out) return CEC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (depth == 0 || depth > 16 || max_entries == 0 || slot_bytes < 16 ||
        max_open > 0xFFFFFFFFull) {
        violation("cec_scrub_pipeline_new: sizes the header refuses");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    auto* pl = new cec_scrub_pipeline{slot_bytes, max_entries, cec::plan::OpenIds(max_open),
                                      std::vector<std::vector<uint8_t>>(max_open),
                                      std::vector<bool>(max_open, false),
                                      std::vector<cec_scrub_pipeline::Slot>(depth), 0};
    g_pipeline = pl;
    *out = pl;
    return CEC_OK;
}
void cec_scrub_pipeline_free(cec_scrub_pipeline* pl) {
    if (g_pipeline == pl) g_pipeline = nullptr;
    delete pl;
}
size_t cec_scrub_pipeline_depth(const cec_scrub_pipeline* pl) { return pl ? pl->slots.size() : 0; }

int cec_scrub_pipeline_acquire(cec_scrub_pipeline* pl, size_t* slot) {
    if (!pl || !slot) return CEC_ERR_INVALID_ARGUMENT;
    cec_scrub_pipeline::Slot& s = pl->slots[pl->next];
    // its previous results are void from here on
    s.in_flight = false;
    s.shown.assign(s.shown.size(), kPoison);
    s.acquired = true;
    *slot = pl->next;
    pl->next = (pl->next + 1) % pl->slots.size();
    return CEC_OK;
}

int cec_scrub_pipeline_submit_from(cec_scrub_pipeline* pl, size_t slot, const uint8_t* const* bufs,
                                   const size_t* lens, const size_t* seg_offsets,
                                   const size_t* seg_lens, const uint32_t* open_ids,
                                   const uint8_t* expected, size_t n) {
    if (!pl || slot >= pl->slots.size() ||
        (n && (!bufs || !lens || !seg_offsets || !seg_lens || !open_ids || !expected)))
        return unreached("cec_scrub_pipeline_submit_from: a null argument or a slot out of range");
    if (n > pl->max_entries) return unreached("a batch of more than max_entries");
    cec_scrub_pipeline::Slot& s = pl->slots[slot];
    if (!s.acquired) return unreached("a slot submitted without being acquired");
    for (size_t k = 0; k < n; ++k)
        if (lens[k] == 0 || seg_lens[k] == 0) {
            violation("a zero length");
            return CEC_EMPTY_SHARD;
        }
    for (size_t k = 0; k < n; ++k)
        if (!bufs[k]) return unreached("a copy is NULL");
    std::vector<uint8_t> flags(n);
    if (const int rule = pl->open.check(lens, seg_offsets, seg_lens, open_ids, n, flags.data())) {
        std::fprintf(stderr, "  contract: the open-id table refuses the batch, rule %d\n", rule);
        ++g_violations;
        return CEC_ERR_INVALID_ARGUMENT;
    }
    size_t bytes = 0;
    for (size_t k = 0; k < n; ++k) bytes += (seg_lens[k] + 15) / 16 * 16;
    if (bytes > pl->slot_bytes) return unreached("a batch beyond the slot's capacity");
    s.acquired = false;  // one batch per acquire
    s.in_flight = true;
    s.hidden.assign(n, kPoison);
    s.shown.assign(n, kPoison);
    ++g_batches;
    g_entries += n;
    g_one_open += pl->open.ids.size() == 1 && n > 1;
    for (size_t k = 0; k < n; ++k) {
        const uint8_t* piece = bufs[k] + seg_offsets[k];
        const bool first = flags[k] & cec::plan::kSegFirst, last = flags[k] & cec::plan::kSegLast;
        uint8_t h[32];
        if (first && last) {
            ++g_whole;
            or_sha256(piece, seg_lens[k], h);
        } else {
            std::vector<uint8_t>& acc = pl->so_far[open_ids[k]];
            if (first) {
                g_reused += pl->id_used[open_ids[k]];
                pl->id_used[open_ids[k]] = true;
                acc.clear();
            } else {
                ++g_continued;
            }
            acc.insert(acc.end(), piece, piece + seg_lens[k]);
            if (!last) continue;
            or_sha256(acc.data(), acc.size(), h);
            acc.clear();
        }
        s.hidden[k] = std::memcmp(h, expected + 32 * k, 32) == 0;  // the one read of row k
    }
    pl->open.commit(lens, seg_offsets, seg_lens, open_ids, flags.data(), n);
    return CEC_OK;
}

int cec_scrub_pipeline_wait(cec_scrub_pipeline* pl, size_t slot, const uint8_t** ok, size_t* n) {
    if (!pl || slot >= pl->slots.size()) return CEC_ERR_INVALID_ARGUMENT;
    cec_scrub_pipeline::Slot& s = pl->slots[slot];
    if (s.in_flight) {
        s.shown = s.hidden;
        s.in_flight = false;
    }
    if (ok) *ok = s.shown.data();
    if (n) *n = s.shown.size();
    return CEC_OK;
}
int cec_scrub_pipeline_query(cec_scrub_pipeline* pl, size_t slot) {
    return pl && slot < pl->slots.size() ? 1 : CEC_ERR_INVALID_ARGUMENT;
}
int cec_scrub_pipeline_drain(cec_scrub_pipeline* pl) {
    return pl ? CEC_OK : CEC_ERR_INVALID_ARGUMENT;
}
size_t cec_scrub_pipeline_open_count(const cec_scrub_pipeline* pl) {
    return pl ? pl->open.count : 0;
}
int cec_scrub_pipeline_abandon(cec_scrub_pipeline* pl, uint32_t id) {
    return pl && pl->open.abandon(id) ? CEC_OK : CEC_ERR_INVALID_ARGUMENT;
}

}  // extern "C"

using namespace chunky_ec;

namespace {

struct Stored {
    FileReference ref;
    std::vector<bool> decodable;  // per part: d or more chunks have a good copy
};

struct World {
    ChunkStore store;
    std::vector<Stored> files;
    std::vector<Location> all_locs;  // every location any chunk lists
    std::set<Location> damaged;      // locations of bad, short and missing copies
    size_t next_loc = 0;
};

// One file of `size` bytes in parts of d * chunk bytes, encoded with the oracle; every chunk
// gets a random mix of locations in the world's store.
void store_file(std::mt19937_64& rng, World& w, size_t d, size_t p, size_t chunk, size_t size) {
    Stored s;
    Bytes bytes(size);
    for (auto& b : bytes) b = uint8_t(rng());
    s.ref.length = size;
    const size_t cap = d * chunk, t = d + p;
    for (size_t off = 0; off < size; off += cap) {
        const size_t len = std::min(cap, size - off), L = (len + d - 1) / d;
        Bytes data(d * L, 0), parity(p * L);
        std::memcpy(data.data(), bytes.data() + off, len);
        std::vector<const uint8_t*> dp(d);
        std::vector<uint8_t*> pp(p);
        std::vector<size_t> dl(d, L), pl(p, L);
        for (size_t i = 0; i < d; ++i) dp[i] = data.data() + i * L;
        for (size_t i = 0; i < p; ++i) pp[i] = parity.data() + i * L;
        if (or_rs_encode_sep(d, p, dp.data(), dl.data(), d, pp.data(), pl.data(), p) != 0)
            violation("oracle encode failed");
        FilePart part;
        part.chunksize = L;
        size_t good_chunks = 0;
        // this part loses more than p chunks now and then, so it cannot be rebuilt
        const bool wreck = rng() % 6 == 0;
        for (size_t i = 0; i < t; ++i) {
            const uint8_t* src = i < d ? dp[i] : pp[i - d];
            std::array<uint8_t, 32> h{};
            or_sha256(src, L, h.data());
            Chunk c{Sha256Hash(h), {}};
            const Bytes good(src, src + L);
            Bytes bad = good;
            bad[rng() % L] ^= 0x40;
            const Bytes shorter(good.begin(), good.end() - 1);
            bool has_good = false;
            auto put_good = [&] {  // the first good copy at the content address, as a write
                Location loc = has_good ? "loc-" + std::to_string(w.next_loc++)
                                        : ChunkStore::location_of(c.hash);
                w.store.put(loc, good);
                c.locations.push_back(loc);
                w.all_locs.push_back(loc);
                has_good = true;
            };
            auto put_damaged = [&](const Bytes* b) {  // nullptr: a location that does not read
                Location loc = "loc-" + std::to_string(w.next_loc++);
                if (b) w.store.put(loc, *b);
                c.locations.push_back(loc);
                w.all_locs.push_back(loc);
                w.damaged.insert(loc);
            };
            switch (wreck ? 8 + rng() % 4 : rng() % 16) {
                case 0: put_damaged(&bad); put_good(); break;
                case 1: put_good(); put_damaged(&bad); break;
                case 2: put_damaged(nullptr); put_damaged(&shorter); put_good(); break;
                case 3: put_good(); put_good(); break;
                case 4: put_damaged(&bad); put_damaged(&bad); break;
                case 5: case 8: put_damaged(&bad); break;
                case 6: case 9: put_damaged(&shorter); break;
                case 7: case 10: put_damaged(nullptr); break;
                default: put_good(); break;
            }
            good_chunks += has_good;
            (i < d ? part.data : part.parity).push_back(std::move(c));
        }
        s.decodable.push_back(good_chunks >= d);
        s.ref.parts.push_back(std::move(part));
    }
    w.files.push_back(std::move(s));
}

bool same_report(const PartReport& a, const PartReport& b) {
    return a.locations == b.locations && a.chunks == b.chunks &&
           a.new_locations == b.new_locations && a.write_error == b.write_error;
}

size_t g_long_copies = 0, g_damaged_parts = 0, g_multi_parts = 0, g_empty_parts = 0;

#define REQUIRE(cond)                                                                \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "  line %d: %s does not hold\n", __LINE__, #cond);  \
            return false;                                                            \
        }                                                                            \
    } while (0)

struct Setting {
    size_t segment, slot, depth, max_open;
};

bool run_seed(uint64_t seed) {
    std::mt19937_64 rng(seed);
    World w;
    const size_t shapes[][2] = {{3, 2}, {10, 4}, {2, 10}};
    const size_t n_files = 1 + rng() % 6;
    for (size_t f = 0; f < n_files; ++f) {
        const auto& sh = shapes[rng() % 3];
        const size_t chunk = size_t(1) << (4 + rng() % 6);  // 16 B .. 512 B
        const size_t kind = rng() % 8;
        const size_t size = kind == 0 ? 0 : 1 + rng() % (kind == 1 ? sh[0] : sh[0] * chunk * 4);
        store_file(rng, w, sh[0], sh[1], chunk, size);
    }
    std::vector<const FileReference*> cptrs;
    std::vector<std::vector<PartReport>> want;
    for (const Stored& s : w.files) {
        cptrs.push_back(&s.ref);
        want.push_back(s.ref.verify(w.store));
        for (size_t k = 0; k < s.ref.parts.size(); ++k) {
            const FilePart& part = s.ref.parts[k];
            g_damaged_parts += !want.back()[k].is_ideal();
            g_empty_parts += part.chunksize == 0;
            bool multi = false;
            for (size_t i = 0; i < part.data.size() + part.parity.size(); ++i)
                multi = multi || part.chunk(i).locations.size() >= 2;
            g_multi_parts += multi;
            g_long_copies += part.chunksize > 64;
        }
    }
    const Setting settings[] = {
        {64, 64, 1, 1},          // a slot of one segment, one copy under way
        {64, 1000, 3, 1},        // one copy under way beside whole ones
        {128, 512, 2, 3},
        {256, 4096, 3, 0},       // as many open as a slot holds segments
        {64, 1 << 16, 2, 0},
        {1024, 1 << 16, 1, 0},   // every copy whole
        {size_t(64) << (rng() % 4), 512 + 16 * size_t(rng() % 200), 1 + size_t(rng() % 4),
         size_t(rng() % 5)},
    };
    for (const Setting& s : settings) {
        // a random max_open of 0 stands for the default, which a slot below a segment makes 0
        if (s.slot < s.segment) continue;
        const auto got = FileReference::verify_many_stream(cptrs, w.store, s.segment, s.slot,
                                                           s.depth, s.max_open);
        REQUIRE(got.size() == want.size());
        for (size_t f = 0; f < want.size(); ++f) {
            REQUIRE(got[f].size() == want[f].size());
            for (size_t k = 0; k < want[f].size(); ++k) REQUIRE(same_report(got[f][k], want[f][k]));
        }
        REQUIRE(!g_pipeline || g_pipeline->open.count == 0);  // no id stays open
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t first = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 0;
    const uint64_t count = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 100;
    size_t failed = 0;
    for (uint64_t s = first; s < first + count; ++s)
        if (!run_seed(s)) {
            std::fprintf(stderr, "seed %llu failed\n", (unsigned long long)s);
            ++failed;
        }
    std::printf("%llu seeds, %zu failed, %d contract violations\n", (unsigned long long)count,
                failed, g_violations);
    std::printf("batches=%zu entries=%zu continued=%zu whole=%zu one_open=%zu reused_ids=%zu\n",
                g_batches, g_entries, g_continued, g_whole, g_one_open, g_reused);
    std::printf("parts: long_copies=%zu damaged=%zu multi_location=%zu empty=%zu\n",
                g_long_copies, g_damaged_parts, g_multi_parts, g_empty_parts);
    return failed || g_violations ? 1 : 0;
}
