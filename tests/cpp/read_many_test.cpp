// read_many_test.cpp — FileReference::read_many against read(), file by file.
//
// read_many gathers every part that is not in a batched run of one shape -- whole small files,
// short last parts, every part when parts_per_batch is 0 -- into ragged batches
// (cec_parts_read); the result must be what read() gives for each file on its own, and the
// files' bytes.  Files: those of write_many_test.cpp (sizes 0, 1, 683, 20480, 3*2^20 + 7 and
// 2*d*chunk + 5), written with write_many.  Every case reads three stores: the store intact, one
// with the first data chunk of every part erased (rebuilt from parity), and one with that chunk's
// copy corrupted (it fails verification, the part is reported short and goes up again with a
// parity chunk).
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_read_many.py runs one process per case, so a crash names its case).
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

struct Written {
    std::vector<Bytes> files;
    std::vector<FileReference> refs;
    ChunkStore store;
};

Written write_files(size_t d, size_t p, size_t chunk) {
    Written w;
    w.files = make_files(d, chunk);
    std::vector<std::pair<const uint8_t*, size_t>> views;
    for (const Bytes& f : w.files) views.emplace_back(f.data(), f.size());
    w.refs = FileWriteBuilder().chunk_size(chunk).data_chunks(d).parity_chunks(p).write_many(
        views, w.store);
    return w;
}

// read_many over the files of `w` from `store` against read() file by file and the bytes.
void compare(const Written& w, const ChunkStore& store, size_t ppb) {
    std::vector<const FileReference*> ptrs;
    for (const FileReference& r : w.refs) ptrs.push_back(&r);
    const std::vector<Bytes> got = FileReference::read_many(ptrs, store, ppb);
    CHECK(got.size() == w.files.size());
    if (got.size() != w.files.size()) return;
    for (size_t f = 0; f < w.files.size(); ++f) {
        CHECK(got[f] == w.files[f]);
        CHECK(got[f] == w.refs[f].read(store, ppb));
    }
}

void three_stores(size_t d, size_t p, size_t chunk, size_t ppb) {
    const Written w = write_files(d, p, chunk);
    compare(w, w.store, ppb);
    ChunkStore erased = w.store, corrupted = w.store;
    size_t n_parts = 0;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts) {
            // the first data chunk holds file bytes, so its location is this part's alone
            const Location& loc = part.chunk(0).locations.at(0);
            CHECK(erased.erase(loc));
            CHECK(corrupted.corrupt(loc, part.chunksize - 1));
            ++n_parts;
        }
    CHECK(n_parts >= 8 && erased.size() + n_parts == w.store.size());
    compare(w, erased, ppb);
    compare(w, corrupted, ppb);
}

void rs32() { three_stores(3, 2, size_t(1) << 10, 0); }

void rs104() { three_stores(10, 4, size_t(1) << 16, 0); }

// parts_per_batch = 8: the runs of two or more parts of one shape go through read_run, every
// other part through the ragged path, in one call.
void mixed_batch() {
    three_stores(3, 2, size_t(1) << 10, 8);
    three_stores(10, 4, size_t(1) << 16, 8);
}

// A part with p + 1 chunks erased: read_many throws what read() throws.
void too_few() {
    const size_t d = 3, p = 2;
    const Written w = write_files(d, p, size_t(1) << 10);
    ChunkStore store = w.store;
    const FilePart& part = w.refs[2].parts.at(0);  // the 683-byte file
    for (size_t i = 0; i < p + 1; ++i) CHECK(store.erase(part.chunk(i + 1).locations.at(0)));
    std::vector<const FileReference*> ptrs;
    for (const FileReference& r : w.refs) ptrs.push_back(&r);
    for (size_t ppb : {size_t(0), size_t(8)}) {
        bool many_threw = false, one_threw = false;
        try {
            FileReference::read_many(ptrs, store, ppb);
        } catch (const ErasureError& e) {
            many_threw = e.error() == Error::TooFewShardsPresent;
        }
        try {
            w.refs[2].read(store, ppb);
        } catch (const ErasureError& e) {
            one_threw = e.error() == Error::TooFewShardsPresent;
        }
        CHECK(many_threw);
        CHECK(one_threw);
    }
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"rs32", rs32},
    {"rs104", rs104},
    {"mixed_batch", mixed_batch},
    {"too_few", too_few},
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
