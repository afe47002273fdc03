// read_many_host_fuzz.cpp — FileReference::read_many's host loop (include/chunky_ec.hpp:
// read_many / read_window: the gathering per (d, p), the draw of d chunks per part, the retry
// rounds with CEC_PRESENT_VERIFIED flags) on the CPU, with cec_parts_read replaced by a stand-in
// that keeps the C-ABI's contract and computes with the oracle (test infrastructure: this binary
// is built and run only by tests/test_cpp_read_many_host.py, plain and under ASan + UBSan).
//
// The stand-in checks what the header promises the engine: a loaded chunk has bytes, every data
// slot of a part is caller memory, CEC_PRESENT_VERIFIED only on chunks an earlier round verified
// for that very slot, never a part resubmitted after it was reported CEC_OK.  It writes only what
// the ABI lets it write: the missing or failed data chunks of decodable parts.
//
// Each seed: a few files of random sizes and shapes, stored with random location mixes (good;
// [bad, good]; [gone, short, good]; bad; gone -- file_part.rs:92-107's location walk).  read_many
// must give the files' bytes, equal to read() file by file, or -- when some part has fewer than d
// chunks with a good copy -- throw TooFewShardsPresent as read() of that file does.
// Usage: read_many_host_fuzz FIRST_SEED N_SEEDS; exit status 0 iff every seed passed.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
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

int g_violations = 0;  // contract breaches seen by the stand-in
size_t g_calls = 0, g_retry_calls = 0;

void violation(const char* what) {
    std::fprintf(stderr, "  contract: %s\n", what);
    ++g_violations;
}

// What the stand-in remembers between the rounds of one read_many: per data-slot-0 pointer (a
// part's place in its file's result identifies it) the chunks it verified and whether it was done.
struct Seen {
    std::vector<uint8_t> verified;
    bool done = false;
};
std::map<const uint8_t*, Seen> g_seen;

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

// The per-part path's calls (read() with parts_per_batch = 0 reads through read_with_context).
int cec_sha256_many(const uint8_t* const* bufs, const size_t* lens, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; ++i) or_sha256(bufs[i], lens[i], out + 32 * i);
    return CEC_OK;
}
int cec_reconstruct_data(const cec_codec* c, uint8_t* const* shards, const size_t* lens,
                         uint8_t* present, size_t n) {
    return or_rs_reconstruct(c->d, c->p, shards, lens, present, n, 1);
}

// The batched runs of read_many (parts_per_batch > 0) go through the scheduler, which
// tests/cpp/host_loop_fuzz.cpp stands in for; this program reads with parts_per_batch = 0, so
// none of these may be reached.
static int unreached(const char* what) {
    violation(what);
    return CEC_ERR_INVALID_ARGUMENT;
}
int cec_reconstruct(const cec_codec*, uint8_t* const*, const size_t*, uint8_t*, size_t) {
    return unreached("cec_reconstruct called");
}
int cec_current_device(int*) { return unreached("cec_current_device called"); }
int cec_host_alloc(size_t, int, void**) { return unreached("cec_host_alloc called"); }
void cec_host_free(void*) { unreached("cec_host_free called"); }
int cec_multi_new(const cec_codec*, size_t, size_t, size_t, const int*, size_t, cec_multi**) {
    return unreached("cec_multi_new called");
}
void cec_multi_free(cec_multi*) { unreached("cec_multi_free called"); }
int cec_multi_read_carry(cec_multi*, const uint8_t*, const uint8_t*, const uint8_t*, size_t,
                         uint8_t*, uint8_t*, int*, const uint8_t**, unsigned, const int32_t*,
                         int32_t*, uint64_t*) {
    return unreached("cec_multi_read_carry called");
}
int cec_multi_carry_release(cec_multi*, int32_t) { return unreached("cec_multi_carry_release called"); }
int cec_multi_wait(cec_multi*, uint64_t) { return unreached("cec_multi_wait called"); }
int cec_multi_query(cec_multi*, uint64_t) { return unreached("cec_multi_query called"); }
const char* cec_multi_last_error(void) { return "no scheduler here"; }

int cec_parts_read(const cec_codec* c, uint8_t* const* shards, const size_t* chunk_lens,
                   size_t n_parts, const uint8_t* present, const uint8_t* expected, int data_only,
                   uint8_t* verified, int* part_status) {
    if (!c || !shards || !chunk_lens || !present || !expected || !verified || !part_status)
        return CEC_ERR_INVALID_ARGUMENT;
    ++g_calls;
    const size_t d = c->d, t = c->d + c->p;
    if (!data_only) violation("read_many reads: data_only expected");
    for (size_t k = 0; k < n_parts; ++k)
        if (chunk_lens[k] == 0) return CEC_EMPTY_SHARD;
    bool retry = false;
    for (size_t k = 0; k < n_parts; ++k) {
        const size_t L = chunk_lens[k];
        uint8_t* const* sh = shards + k * t;
        const uint8_t* pr = present + k * t;
        for (size_t i = 0; i < t; ++i)
            if ((pr[i] || i < d) && !sh[i]) {
                violation("a loaded chunk or a data slot is NULL");
                return CEC_ERR_INVALID_ARGUMENT;
            }
        Seen& seen = g_seen[sh[0]];
        if (seen.verified.empty()) seen.verified.assign(t, 0);
        else retry = true;
        if (seen.verified.size() != t) violation("a part's place reused with another shape");
        if (seen.done) violation("a part reported CEC_OK was submitted again");
        size_t good = 0;
        std::vector<uint8_t> ok(t, 0);
        for (size_t i = 0; i < t; ++i) {
            if (pr[i] == CEC_PRESENT_VERIFIED) {
                if (!seen.verified[i]) violation("CEC_PRESENT_VERIFIED on a chunk never verified");
                ok[i] = 1;
            } else if (pr[i]) {
                if (seen.verified[i]) violation("a verified chunk was loaded and hashed again");
                uint8_t h[32];
                or_sha256(sh[i], L, h);
                ok[i] = std::memcmp(h, expected + (k * t + i) * 32, 32) == 0;
            }
            good += ok[i];
        }
        for (size_t i = 0; i < t; ++i) {
            verified[k * t + i] = ok[i];
            seen.verified[i] = seen.verified[i] || ok[i];
        }
        if (good < d) {
            part_status[k] = CEC_TOO_FEW_SHARDS_PRESENT;
            continue;
        }
        part_status[k] = CEC_OK;
        seen.done = true;
        // rebuild from the verified chunks into the data slots that did not verify; parity slots
        // that were not loaded may be NULL and are never touched under data_only
        std::vector<uint8_t*> ptrs(sh, sh + t);
        std::vector<size_t> lens(t, L);
        const int st = or_rs_reconstruct(d, c->p, ptrs.data(), lens.data(), ok.data(), t, 1);
        if (st != 0) violation("oracle reconstruct failed");
    }
    if (retry) ++g_retry_calls;
    return CEC_OK;
}

}  // extern "C"

using namespace chunky_ec;

namespace {

struct Stored {
    FileReference ref;
    Bytes bytes;
    bool readable = true;  // every part has d chunks with a good copy
};

// One file of `size` bytes in parts of d * chunk bytes, encoded with the oracle; every chunk
// gets a random mix of locations in `store`.
Stored store_file(std::mt19937_64& rng, ChunkStore& store, size_t d, size_t p, size_t chunk,
                  size_t size, size_t* next_loc) {
    Stored s;
    s.bytes.resize(size);
    for (auto& b : s.bytes) b = uint8_t(rng());
    s.ref.length = size;
    const size_t cap = d * chunk, t = d + p;
    for (size_t off = 0; off < size; off += cap) {
        const size_t len = std::min(cap, size - off), L = (len + d - 1) / d;
        Bytes data(d * L, 0), parity(p * L);
        std::memcpy(data.data(), s.bytes.data() + off, len);
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
        for (size_t i = 0; i < t; ++i) {
            const uint8_t* src = i < d ? dp[i] : pp[i - d];
            std::array<uint8_t, 32> h{};
            or_sha256(src, L, h.data());
            Chunk c{Sha256Hash(h), {}};
            const Bytes good(src, src + L);
            Bytes bad = good;
            bad[rng() % L] ^= 0x40;
            auto put = [&](const Bytes* b) {  // nullptr: a location that does not read
                Location loc = "loc-" + std::to_string((*next_loc)++);
                if (b) store.put(loc, *b);
                c.locations.push_back(loc);
            };
            bool has_good = true;
            switch (rng() % 8) {
                case 0: put(&bad); put(&good); break;
                case 1: {
                    const Bytes shorter(good.begin(), good.end() - 1);
                    put(nullptr); put(&shorter); put(&good);
                    break;
                }
                case 2: put(&bad); has_good = false; break;
                case 3: put(nullptr); has_good = false; break;
                default: put(&good); break;
            }
            good_chunks += has_good;
            (i < d ? part.data : part.parity).push_back(std::move(c));
        }
        if (good_chunks < d) s.readable = false;
        s.ref.parts.push_back(std::move(part));
    }
    return s;
}

bool throws_too_few(const std::function<void()>& fn) {
    try {
        fn();
    } catch (const ErasureError& e) {
        return e.error() == Error::TooFewShardsPresent;
    }
    return false;
}

bool run_seed(uint64_t seed) {
    std::mt19937_64 rng(seed);
    ChunkStore store;
    size_t next_loc = 0;
    const size_t shapes[][2] = {{1, 1}, {3, 2}, {10, 4}, {2, 10}};
    std::vector<Stored> files;
    const size_t n_files = 1 + rng() % 6;
    for (size_t f = 0; f < n_files; ++f) {
        const auto& sh = shapes[rng() % 4];
        const size_t chunk = size_t(1) << (4 + rng() % 6);  // 16 B .. 512 B
        const size_t size = rng() % 8 == 0 ? 0 : 1 + rng() % (sh[0] * chunk * 4);
        files.push_back(store_file(rng, store, sh[0], sh[1], chunk, size, &next_loc));
    }
    std::vector<const FileReference*> ptrs;
    bool all_readable = true;
    for (const Stored& s : files) {
        ptrs.push_back(&s.ref);
        all_readable = all_readable && s.readable;
    }
    g_seen.clear();
    bool ok = true;
    if (all_readable) {
        const std::vector<Bytes> got = FileReference::read_many(ptrs, store);
        ok = got.size() == files.size();
        for (size_t f = 0; ok && f < files.size(); ++f)
            ok = got[f] == files[f].bytes && got[f] == files[f].ref.read(store);
    } else {
        ok = throws_too_few([&] { FileReference::read_many(ptrs, store); });
        for (const Stored& s : files)
            if (!s.readable) ok = ok && throws_too_few([&] { s.ref.read(store); });
    }
    if (!ok) std::fprintf(stderr, "seed %llu failed\n", (unsigned long long)seed);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t first = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 0;
    const uint64_t count = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 100;
    size_t failed = 0;
    for (uint64_t s = first; s < first + count; ++s) failed += run_seed(s) ? 0 : 1;
    std::printf("%llu seeds, %zu failed, %d contract violations, %zu engine calls (%zu with "
                "retried parts)\n",
                (unsigned long long)count, failed, g_violations, g_calls, g_retry_calls);
    return failed || g_violations ? 1 : 0;
}
