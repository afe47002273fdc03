// check_many_host_fuzz.cpp — FileReference::verify_many / resilver_many's host loops
// (include/chunky_ec.hpp: the gathering into windows, the report skeleton, the prepass over chunks
// with several locations, the CEC_PRESENT_VERIFIED flags, the write-backs) on the CPU, with
// cec_parts_verify and cec_parts_read replaced by stand-ins that keep the C-ABI's contract and
// compute with the oracle (test infrastructure: this binary is built and run only by
// tests/test_cpp_check_many_host.py, plain and under ASan + UBSan).
//
// The stand-ins count what the header promises the engine and breaks: a needed slot that is
// NULL, a zero length, a CEC_PRESENT_VERIFIED flag on bytes that do not hash to the digest, a
// copy hashed twice across a resilver window's two calls (a lone copy in the prepass, or a copy
// of a chunk with several locations hashed again by the read call), a part submitted twice.
//
// Each seed: a few files of random sizes (0 up to a few parts) and shapes RS(3,2), RS(10,4),
// RS(2,10), every chunk stored with a random mix of locations: good; [bad, good]; [good, bad];
// [gone, short, good]; [good, good]; [bad, bad]; bad; short; gone.  A chunk's first good copy
// lies at its content address, as a write puts it there, so identical chunks (zero padding)
// share that location; every damaged copy has a location of its own, which the program asserts.
// Checked: verify_many equals verify() file by file; resilver_many on one copy of the store
// equals resilver() file by file on another (reports, the files' location lists, the final
// store); every location the resilver did not write holds its earlier bytes; a later verify_many
// is ideal for every part that had d valid chunks.
// Usage: check_many_host_fuzz FIRST_SEED N_SEEDS; exit status 0 iff every seed passed.
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

extern "C" {
// oracle/cec_oracle.c
void or_sha256(const uint8_t* buf, size_t len, uint8_t out[32]);
int or_rs_encode_sep(size_t d, size_t p, const uint8_t* const* data, const size_t* data_lens,
                     size_t n_data, uint8_t* const* parity, const size_t* parity_lens,
                     size_t n_parity);
int or_rs_reconstruct(size_t d, size_t p, uint8_t* const* shards, const size_t* lens,
                      uint8_t* present, size_t n_shards, int data_only);
}

namespace {

int g_violations = 0;  // contract breaches seen by the stand-ins
size_t g_verify_calls = 0, g_read_calls = 0;

void violation(const char* what) {
    std::fprintf(stderr, "  contract: %s\n", what);
    ++g_violations;
}

using Digest = std::string;  // 32 raw bytes

// What the program tells the stand-ins about the call in progress.
bool g_resilver = false;         // inside resilver_many (else verify_many)
std::set<Digest> g_multi;        // digests of chunks with two or more locations
std::set<Digest> g_lone;         // digests of chunks with exactly one
std::map<std::string, int> g_parts_allowed, g_parts_seen;  // per part key (its t digests)

}  // namespace

struct cec_codec {
    size_t d, p;
};

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

// The per-part path's calls: verify() and resilver() with parts_per_batch = 0 hash through
// check_locations and rebuild through ReedSolomon::reconstruct.  Called from several threads.
int cec_sha256_many(const uint8_t* const* bufs, const size_t* lens, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; ++i) or_sha256(bufs[i], lens[i], out + 32 * i);
    return CEC_OK;
}
int cec_reconstruct(const cec_codec* c, uint8_t* const* shards, const size_t* lens,
                    uint8_t* present, size_t n) {
    return or_rs_reconstruct(c->d, c->p, shards, lens, present, n, 0);
}

// The batched runs (parts_per_batch > 0) go through the scheduler, which
// tests/cpp/host_loop_fuzz.cpp stands in for; this program passes parts_per_batch = 0, so none of
// these may be reached.
static int unreached(const char* what) {
    violation(what);
    return CEC_ERR_INVALID_ARGUMENT;
}
int cec_reconstruct_data(const cec_codec*, uint8_t* const*, const size_t*, uint8_t*, size_t) {
    return unreached("cec_reconstruct_data called");  // nothing here reads
}
int cec_current_device(int*) { return unreached("cec_current_device called"); }
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

int cec_parts_verify(const uint8_t* const* bufs, const size_t* lens, size_t n,
                     const uint8_t* expected, uint8_t* ok) {
    if (n == 0) return CEC_OK;
    if (!bufs || !lens || !expected || !ok) return CEC_ERR_INVALID_ARGUMENT;
    ++g_verify_calls;
    for (size_t i = 0; i < n; ++i)
        if (lens[i] == 0) {
            violation("cec_parts_verify: a zero length");
            return CEC_EMPTY_SHARD;
        }
    for (size_t i = 0; i < n; ++i)
        if (!bufs[i]) {
            violation("cec_parts_verify: a copy is NULL");
            return CEC_ERR_INVALID_ARGUMENT;
        }
    for (size_t i = 0; i < n; ++i) {
        const Digest want(reinterpret_cast<const char*>(expected + 32 * i), 32);
        // a resilver window's prepass hashes the copies of chunks with several locations only:
        // a lone copy is hashed by the read call behind it
        if (g_resilver && !g_multi.count(want))
            violation("a lone copy was hashed in the prepass and again by the read call");
        uint8_t h[32];
        or_sha256(bufs[i], lens[i], h);
        ok[i] = std::memcmp(h, want.data(), 32) == 0;
    }
    return CEC_OK;
}

int cec_parts_read(const cec_codec* c, uint8_t* const* shards, const size_t* chunk_lens,
                   size_t n_parts, const uint8_t* present, const uint8_t* expected, int data_only,
                   uint8_t* verified, int* part_status) {
    if (!c) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!shards || !chunk_lens || !present || !expected || !verified || !part_status)
        return CEC_ERR_INVALID_ARGUMENT;
    ++g_read_calls;
    const size_t d = c->d, t = c->d + c->p;
    if (data_only) violation("resilver_many rebuilds data and parity: data_only = 0 expected");
    if (!g_resilver) violation("cec_parts_read called outside resilver_many");
    for (size_t k = 0; k < n_parts; ++k)
        if (chunk_lens[k] == 0) {
            violation("cec_parts_read: a zero length");
            return CEC_EMPTY_SHARD;
        }
    for (size_t k = 0; k < n_parts; ++k) {
        size_t loaded = 0;
        for (size_t i = 0; i < t; ++i) loaded += present[k * t + i] ? 1 : 0;
        for (size_t i = 0; i < t; ++i)
            if ((present[k * t + i] || loaded >= d) && !shards[k * t + i]) {
                violation("a chunk slot that is read or filled is NULL");
                return CEC_ERR_INVALID_ARGUMENT;
            }
    }
    for (size_t k = 0; k < n_parts; ++k) {
        const size_t L = chunk_lens[k];
        uint8_t* const* sh = shards + k * t;
        const uint8_t* pr = present + k * t;
        const std::string key(reinterpret_cast<const char*>(expected + k * t * 32), t * 32);
        if (++g_parts_seen[key] > g_parts_allowed[key]) violation("a part was submitted twice");
        size_t good = 0;
        std::vector<uint8_t> ok(t, 0);
        for (size_t i = 0; i < t; ++i) {
            if (!pr[i]) continue;
            const Digest want(reinterpret_cast<const char*>(expected + (k * t + i) * 32), 32);
            uint8_t h[32];
            or_sha256(sh[i], L, h);
            const bool same = std::memcmp(h, want.data(), 32) == 0;
            if (pr[i] == CEC_PRESENT_VERIFIED) {
                if (!same) violation("CEC_PRESENT_VERIFIED on bytes that do not hash to the digest");
                ok[i] = 1;  // trusted, as the engine trusts it
            } else {
                // the copies of a chunk with several locations were hashed by the prepass
                if (g_multi.count(want) && !g_lone.count(want))
                    violation("a copy the prepass hashed was hashed again by the read call");
                ok[i] = same;
            }
            good += ok[i];
        }
        for (size_t i = 0; i < t; ++i) verified[k * t + i] = ok[i];
        if (good < d) {
            part_status[k] = CEC_TOO_FEW_SHARDS_PRESENT;  // nothing of it is written
            continue;
        }
        part_status[k] = CEC_OK;
        // every chunk that did not verify is rebuilt into its own slot
        std::vector<uint8_t*> ptrs(sh, sh + t);
        std::vector<size_t> lens(t, L);
        if (or_rs_reconstruct(d, c->p, ptrs.data(), lens.data(), ok.data(), t, 0) != 0)
            violation("oracle reconstruct failed");
    }
    return CEC_OK;
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

Digest digest_of(const Chunk& c) {
    return Digest(reinterpret_cast<const char*>(c.hash.digest().data()), 32);
}

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

bool same_bytes(const ChunkStore& a, const ChunkStore& b, const Location& loc) {
    const Bytes *x = a.find(loc), *y = b.find(loc);
    return (!x && !y) || (x && y && *x == *y);
}

size_t g_multi_parts = 0, g_rebuilt_parts = 0, g_error_parts = 0, g_shared_locs = 0;

#define REQUIRE(cond)                                                                \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "  line %d: %s does not hold\n", __LINE__, #cond);  \
            return false;                                                            \
        }                                                                            \
    } while (0)

bool run_seed(uint64_t seed) {
    std::mt19937_64 rng(seed);
    World w;
    const size_t shapes[][2] = {{3, 2}, {10, 4}, {2, 10}};
    const size_t n_files = 1 + rng() % 6;
    for (size_t f = 0; f < n_files; ++f) {
        const auto& sh = shapes[rng() % 3];
        const size_t chunk = size_t(1) << (4 + rng() % 6);  // 16 B .. 512 B
        // empty now and then; a few bytes now and then (one-byte chunks, most of them the zero
        // padding, which share their location); else up to four parts
        const size_t kind = rng() % 8;
        const size_t size = kind == 0 ? 0 : 1 + rng() % (kind == 1 ? sh[0] : sh[0] * chunk * 4);
        store_file(rng, w, sh[0], sh[1], chunk, size);
    }
    // the damage never touches a location that two chunks share
    std::map<Location, size_t> refs;
    for (const Location& loc : w.all_locs) ++refs[loc];
    for (const Location& loc : w.damaged) REQUIRE(refs[loc] == 1);
    for (const auto& kv : refs) g_shared_locs += kv.second > 1;
    // what the stand-ins are told: the digests of chunks with one / several locations, the parts
    g_multi.clear();
    g_lone.clear();
    g_parts_allowed.clear();
    for (const Stored& s : w.files)
        for (const FilePart& part : s.ref.parts) {
            std::string key;
            const size_t t = part.data.size() + part.parity.size();
            for (size_t i = 0; i < t; ++i) {
                const Chunk& c = part.chunk(i);
                (c.locations.size() >= 2 ? g_multi : g_lone).insert(digest_of(c));
                key += digest_of(c);
            }
            ++g_parts_allowed[key];
        }

    // verify_many against verify(), file by file
    std::vector<const FileReference*> cptrs;
    for (const Stored& s : w.files) cptrs.push_back(&s.ref);
    g_resilver = false;
    const auto verified = FileReference::verify_many(cptrs, w.store);
    REQUIRE(verified.size() == w.files.size());
    for (size_t f = 0; f < w.files.size(); ++f) {
        const std::vector<PartReport> one = w.files[f].ref.verify(w.store);
        REQUIRE(verified[f].size() == one.size());
        for (size_t k = 0; k < one.size(); ++k) REQUIRE(same_report(verified[f][k], one[k]));
    }

    // resilver_many on one copy of the store against resilver() file by file on another
    ChunkStore many_store = w.store, one_store = w.store;
    std::vector<FileReference> many_refs, one_refs;
    for (const Stored& s : w.files) {
        many_refs.push_back(s.ref);
        one_refs.push_back(s.ref);
    }
    std::vector<FileReference*> mptrs;
    for (FileReference& r : many_refs) mptrs.push_back(&r);
    std::vector<Location> written;
    many_store.log_writes(&written);
    g_resilver = true;
    g_parts_seen.clear();
    const auto resilvered = FileReference::resilver_many(mptrs, many_store);
    g_resilver = false;
    many_store.log_writes(nullptr);
    REQUIRE(resilvered.size() == w.files.size());
    for (size_t f = 0; f < w.files.size(); ++f) {
        const std::vector<PartReport> one = one_refs[f].resilver(one_store);
        REQUIRE(resilvered[f].size() == one.size());
        for (size_t k = 0; k < one.size(); ++k) {
            REQUIRE(same_report(resilvered[f][k], one[k]));
            const FilePart &a = many_refs[f].parts[k], &b = one_refs[f].parts[k];
            const size_t t = a.data.size() + a.parity.size();
            bool multi = false;
            for (size_t i = 0; i < t; ++i) {
                REQUIRE(a.chunk(i).locations == b.chunk(i).locations);
                multi = multi || w.files[f].ref.parts[k].chunk(i).locations.size() >= 2;
            }
            g_multi_parts += multi;
            g_rebuilt_parts += !one[k].new_locations.empty();
            g_error_parts += one[k].write_error.has_value();
            REQUIRE(one[k].write_error.has_value() == !w.files[f].decodable[k]);
        }
    }
    // the final stores are equal; what the resilver did not write holds its earlier bytes
    REQUIRE(many_store.size() == one_store.size());
    const std::set<Location> wrote(written.begin(), written.end());
    for (const Location& loc : wrote) REQUIRE(same_bytes(many_store, one_store, loc));
    for (const Location& loc : w.all_locs) {
        REQUIRE(same_bytes(many_store, one_store, loc));
        if (!wrote.count(loc)) REQUIRE(same_bytes(many_store, w.store, loc));
    }
    REQUIRE(many_store.size() >= w.store.size() && many_store.size() <= w.store.size() + wrote.size());

    // afterwards every part that had d valid chunks is ideal
    std::vector<const FileReference*> aptrs;
    for (const FileReference& r : many_refs) aptrs.push_back(&r);
    const auto after = FileReference::verify_many(aptrs, many_store);
    for (size_t f = 0; f < w.files.size(); ++f)
        for (size_t k = 0; k < after[f].size(); ++k)
            if (w.files[f].decodable[k]) REQUIRE(after[f][k].is_ideal());
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
    std::printf("%llu seeds, %zu failed, %d contract violations, %zu verify calls, %zu read calls\n",
                (unsigned long long)count, failed, g_violations, g_verify_calls, g_read_calls);
    std::printf("parts: multi_location=%zu rebuilt=%zu write_error=%zu shared_locations=%zu\n",
                g_multi_parts, g_rebuilt_parts, g_error_parts, g_shared_locs);
    return failed || g_violations ? 1 : 0;
}
