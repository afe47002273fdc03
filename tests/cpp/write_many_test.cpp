// write_many_test.cpp — FileWriteBuilder::write_many against write(), file by file.
//
// write_many gathers every part that is not a full part of a batched file -- whole small files,
// short last parts -- into ragged batches (cec_parts_encode); the result must be what write()
// gives for each file on its own: the same FileReference (parts, chunksize, digests, locations,
// length), the same stored chunks, and the chunks handed to the store in file, part, chunk
// order.  Files: sizes 0, 1, 683, 20480 (the tests/cluster.rs generator), 3*2^20 + 7 and
// 2*d*chunk + 5.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_write_many.py runs one process per case, so a crash names its case).
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

// tests/cluster.rs:95-102: 80 blocks of 256 bytes, byte x of block i = (x % 128) + i.
Bytes cluster_reader_bytes() {
    Bytes b;
    for (int i = 0; i < 80; ++i)
        for (int x = 0; x < 256; ++x) b.push_back(uint8_t((x % 128) + i));
    return b;
}

std::vector<Bytes> make_files(size_t d, size_t chunk) {
    std::vector<Bytes> files;
    files.push_back(Bytes());
    files.push_back(random_bytes(1, 1));
    files.push_back(random_bytes(683, 2));
    files.push_back(cluster_reader_bytes());
    files.push_back(random_bytes(3 * (size_t(1) << 20) + 7, 3));
    files.push_back(random_bytes(2 * d * chunk + 5, 4));
    return files;
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

// write_many over the files against write() file by file, with `builder`.
void compare(const FileWriteBuilder& builder, size_t d, size_t chunk) {
    const std::vector<Bytes> files = make_files(d, chunk);
    std::vector<std::pair<const uint8_t*, size_t>> views;
    for (const Bytes& f : files) views.emplace_back(f.data(), f.size());

    ChunkStore one_store, many_store;
    std::vector<Location> one_log, many_log;
    one_store.log_writes(&one_log);
    many_store.log_writes(&many_log);
    std::vector<FileReference> want;
    for (const Bytes& f : files) want.push_back(builder.write(f, one_store));
    const std::vector<FileReference> got = builder.write_many(views, many_store);
    one_store.log_writes(nullptr);
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
        // bit-exact through the per-part read
        CHECK(got[f].read(many_store) == files[f]);
    }
    CHECK(many_store.size() == one_store.size());
    // write_shard calls in file, part, chunk order.  (write() itself hands the parts of one
    // file to `concurrency` tasks, so its own log is in file order only; the order write_many
    // promises is the FileReferences'.)
    CHECK(many_log == ref_order);
    CHECK(many_log.size() == one_log.size());
}

void rs32() {
    compare(FileWriteBuilder().chunk_size(size_t(1) << 10).data_chunks(3).parity_chunks(2), 3,
            size_t(1) << 10);
}

void rs104() {
    compare(FileWriteBuilder().chunk_size(size_t(1) << 16).data_chunks(10).parity_chunks(4), 10,
            size_t(1) << 16);
}

// batch(8, 3): the files with two or more full parts send those through the batched full-parts
// path, everything else through the ragged path, in one call.
void mixed_batch() {
    compare(FileWriteBuilder().chunk_size(size_t(1) << 10).data_chunks(3).parity_chunks(2).batch(8, 3),
            3, size_t(1) << 10);
    compare(FileWriteBuilder().chunk_size(size_t(1) << 16).data_chunks(10).parity_chunks(4).batch(8, 3),
            10, size_t(1) << 16);
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"rs32", rs32},
    {"rs104", rs104},
    {"mixed_batch", mixed_batch},
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
