// write_many_segments_test.cpp — FileWriteBuilder::write_many_stream under many_segment(128)
// against write(), file by file.
//
// With many_segment set, a gathered part whose chunks are longer than the segment goes through
// the calling thread's segment pipeline (cec_segment_pipeline_*) as column segments, one per
// batch, with short parts in the same batches.  The result must be what write() gives for each
// file on its own: the same FileReference (parts, chunksize, digests, locations, length), the same
// stored chunks, and the chunks handed to the store in file, part, chunk order, also where a
// short part is complete long before a long one in front of it.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_write_many_segments.py runs one process per case, so a crash names its case).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "chunky_ec.hpp"

using namespace chunky_ec;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "  %s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                       \
        }                                                                       \
    } while (0)

constexpr size_t kSegment = 128, kChunk = 1024;

Bytes random_bytes(size_t n, uint64_t seed) {
    Bytes b(n);
    uint64_t z = seed * 0x2545F4914F6CDD1Dull + 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n; ++i) {
        z ^= z << 13;
        z ^= z >> 7;
        z ^= z << 17;
        b[i] = uint8_t(z >> 24);
    }
    return b;
}

bool same_part(const FilePart& a, const FilePart& b) {
    if (a.chunksize != b.chunksize || a.data.size() != b.data.size() ||
        a.parity.size() != b.parity.size())
        return false;
    for (size_t i = 0; i < a.data.size() + a.parity.size(); ++i)
        if (!(a.chunk(i).hash == b.chunk(i).hash) || a.chunk(i).locations != b.chunk(i).locations)
            return false;
    return true;
}

// write_many_stream over the files against write() file by file, with `builder`.
void compare(const FileWriteBuilder& builder, const std::vector<Bytes>& files) {
    std::vector<std::pair<const uint8_t*, size_t>> views;
    for (const Bytes& f : files) views.emplace_back(f.data(), f.size());

    ChunkStore one_store, many_store;
    std::vector<Location> many_log;
    many_store.log_writes(&many_log);
    std::vector<FileReference> want;
    for (const Bytes& f : files) want.push_back(builder.write(f, one_store));
    const std::vector<FileReference> got = builder.write_many_stream(views, many_store);
    many_store.log_writes(nullptr);

    CHECK(got.size() == files.size());
    if (got.size() != files.size()) return;
    std::vector<Location> ref_order;  // file, part, chunk
    for (size_t f = 0; f < files.size(); ++f) {
        CHECK(got[f].length && *got[f].length == files[f].size());
        CHECK(got[f].length == want[f].length);
        CHECK(got[f].parts.size() == want[f].parts.size());
        if (got[f].parts.size() != want[f].parts.size()) continue;
        if (files[f].empty()) CHECK(got[f].parts.empty());
        for (size_t k = 0; k < got[f].parts.size(); ++k) {
            CHECK(same_part(got[f].parts[k], want[f].parts[k]));
            const FilePart& part = got[f].parts[k];
            for (size_t i = 0; i < part.data.size() + part.parity.size(); ++i) {
                const Location& loc = part.chunk(i).locations.at(0);
                ref_order.push_back(loc);
                const Bytes* a = many_store.find(loc);
                const Bytes* b = one_store.find(loc);
                CHECK(a && b && *a == *b && a->size() == part.chunksize);
            }
        }
        CHECK(got[f].read(many_store) == files[f]);  // bit-exact through the per-part read
    }
    CHECK(many_store.size() == one_store.size());
    CHECK(many_log == ref_order);  // write_shard calls in file, part, chunk order
}

FileWriteBuilder builder(size_t d, size_t p, size_t max_open = 0) {
    FileWriteBuilder b;
    b.chunk_size(kChunk).data_chunks(d).parity_chunks(p).many_slots(size_t(16) << 10, 2)
        .many_segment(kSegment, max_open);
    return b;
}

// Long parts (chunks of up to 1 KiB: eight segments) between short ones (whole parts), sizes that
// are no multiple of anything, files of several parts: short parts are complete while long ones
// in front of them are still open and are held back.
std::vector<Bytes> mixed_files(size_t d, size_t count) {
    std::vector<Bytes> files;
    uint64_t z = 4242 + d;
    for (size_t f = 0; f < count; ++f) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        const size_t r = (z >> 33);
        const size_t size = f % 3 == 0   ? d * 300 + r % (d * 700)  // one long part
                            : f % 3 == 1 ? 1 + r % (d * kSegment)   // one whole part
                                         : d * kChunk + 1 + r % (2 * d * kChunk);  // 2-3 parts
        files.push_back(random_bytes(size, f + 1));
    }
    return files;
}

void long_and_short_interleaved() {
    compare(builder(3, 2), mixed_files(3, 40));
    compare(builder(10, 4), mixed_files(10, 25));
}

// Chunk lengths that are exact multiples of the segment (the last segment is a whole one), the
// segment itself (a whole part), and one byte more and less.
void exact_multiples_of_the_segment() {
    const size_t d = 3;
    std::vector<Bytes> files;
    uint64_t seed = 100;
    for (size_t L : {kSegment, 2 * kSegment, 3 * kSegment, kChunk, kSegment + 1, kSegment - 1,
                     2 * kSegment + 1, 2 * kSegment - 1})
        for (size_t cut : {size_t(0), size_t(1), d - 1})  // the last data chunk padded or not
            files.push_back(random_bytes(d * L - cut, ++seed));
    compare(builder(3, 2), files);
}

void empty_files() {
    compare(builder(3, 2), {Bytes()});
    compare(builder(3, 2), {Bytes(), random_bytes(3 * 700, 5), Bytes(), random_bytes(7, 6), Bytes()});
    compare(builder(3, 2), {});
}

// A file with three full parts and a tail between the others, batch() set: its full parts go
// through the batched full-parts path after everything before them has reached the store.
void full_parts_in_the_middle() {
    for (const auto& shape : {std::pair<size_t, size_t>{3, 2}, {10, 4}}) {
        const size_t d = shape.first;
        std::vector<Bytes> files = mixed_files(d, 12);
        files.insert(files.begin() + 5, random_bytes(3 * d * kChunk + 4321, 77));
        files.insert(files.begin() + 9, random_bytes(2 * d * kChunk, 78));
        FileWriteBuilder b = builder(d, shape.second);
        b.batch(8, 3);
        compare(b, files);
    }
}

// More long parts than open ids: new long parts wait for an id while short parts behind them
// cannot overtake, with one id and with two.
void max_open_reached() {
    std::vector<Bytes> files;
    for (size_t f = 0; f < 12; ++f)
        files.push_back(random_bytes(f % 4 == 3 ? 50 + f : 3 * (400 + 37 * f), 200 + f));
    compare(builder(3, 2, 1), files);
    compare(builder(3, 2, 2), files);
}

// The option is off by default and 0 turns it off again; a bad value is refused.
void option_rules() {
    bool threw = false;
    try {
        FileWriteBuilder().many_segment(100);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw);
    FileWriteBuilder off = builder(3, 2);
    off.many_segment(0);
    compare(off, mixed_files(3, 9));
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"long_and_short_interleaved", long_and_short_interleaved},
    {"exact_multiples_of_the_segment", exact_multiples_of_the_segment},
    {"empty_files", empty_files},
    {"full_parts_in_the_middle", full_parts_in_the_middle},
    {"max_open_reached", max_open_reached},
    {"option_rules", option_rules},
};

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (const Case& c : kCases) std::printf("%s\n", c.name);
        return 0;
    }
    int failed = 0, ran = 0;
    for (const Case& c : kCases) {
        if (argc > 1 && std::strcmp(argv[1], c.name) != 0) continue;
        ++ran;
        const int before = g_failures;
        try {
            c.fn();
        } catch (const std::exception& e) {
            std::fprintf(stderr, "  exception: %s\n", e.what());
            ++g_failures;
        }
        const bool ok = g_failures == before;
        failed += ok ? 0 : 1;
        std::printf("%s ... %s\n", c.name, ok ? "ok" : "FAILED");
        std::fflush(stdout);
    }
    if (ran == 0) {
        std::fprintf(stderr, "no such case\n");
        return 2;
    }
    std::printf("%s\n", failed ? "FAILED" : "all passed");
    return failed ? 1 : 0;
}
