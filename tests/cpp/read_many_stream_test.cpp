// read_many_stream_test.cpp — FileReference::read_many_stream against read_many and the files'
// bytes.
//
// read_many_stream gathers the windows read_many gathers, but a window is a batch of a ragged
// read pipeline (cec_parts_reader_*) with several in flight, and the parts a batch reports short
// go up again as a later batch.  Whatever the store looks like, the result must be read_many's
// and the written bytes, and a part whose copies run out must fail the same way.  Files: 1 byte
// to a few MiB, at RS(3,2) and RS(10,4); reader depths 1 and 3.  Stores: intact, the first data
// chunk of every part erased, that chunk corrupted, and 1 % of all copies corrupted (seeded), so
// that parts need retry rounds while other batches are in flight.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_read_many_stream.py runs one process per case, so a crash names its case).
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

uint64_t next(uint64_t& z) {
    z ^= z << 13;
    z ^= z >> 7;
    z ^= z << 17;
    return z;
}

Bytes random_bytes(size_t n, uint64_t seed) {
    Bytes b(n);
    uint64_t z = seed * 0x2545F4914F6CDD1Dull + 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n; ++i) b[i] = uint8_t(next(z) >> 24);
    return b;
}

// 1 byte, the boundaries of a part, 120 seeded sizes below 64 KiB, and two files of a few MiB.
std::vector<Bytes> make_files(size_t d, size_t chunk) {
    std::vector<Bytes> files;
    uint64_t seed = 1;
    for (size_t n : {size_t(1), size_t(683), d * chunk - 1, d * chunk, d * chunk + 1})
        files.push_back(random_bytes(n, seed++));
    uint64_t z = 0x1234567ull + d;
    for (int i = 0; i < 120; ++i) files.push_back(random_bytes(1 + next(z) % 65536, seed++));
    files.push_back(random_bytes(3 * (size_t(1) << 20) + 7, seed++));
    files.push_back(random_bytes(2 * (size_t(1) << 20) + 4097, seed++));
    return files;
}

struct Written {
    std::vector<Bytes> files;
    std::vector<FileReference> refs;
    ChunkStore store;
    std::vector<const FileReference*> ptrs() const {
        std::vector<const FileReference*> out;
        for (const FileReference& r : refs) out.push_back(&r);
        return out;
    }
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

// read_many_stream at reader depths 1 and 3 against read_many and the bytes.
void compare(const Written& w, const ChunkStore& store, size_t ppb,
             size_t slot_bytes = size_t(64) << 20) {
    const std::vector<const FileReference*> ptrs = w.ptrs();
    const std::vector<Bytes> want = FileReference::read_many(ptrs, store, ppb);
    CHECK(want.size() == w.files.size());
    for (size_t depth : {size_t(1), size_t(3)}) {
        const std::vector<Bytes> got =
            FileReference::read_many_stream(ptrs, store, ppb, 4, {}, depth, slot_bytes);
        CHECK(got.size() == w.files.size());
        if (got.size() != w.files.size() || want.size() != got.size()) return;
        for (size_t f = 0; f < w.files.size(); ++f) {
            CHECK(got[f] == w.files[f]);
            CHECK(got[f] == want[f]);
        }
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
    CHECK(n_parts >= 128 && erased.size() + n_parts == w.store.size());
    compare(w, erased, ppb);
    compare(w, corrupted, ppb);
}

void rs32() { three_stores(3, 2, size_t(1) << 12, 0); }

void rs104() { three_stores(10, 4, size_t(1) << 16, 0); }

// parts_per_batch = 8: the runs of two or more parts of one shape go through read_run, every
// other part through the reader, in one call.
void mixed_batch() { three_stores(3, 2, size_t(1) << 12, 8); }

// 1 % of all copies corrupted: the parts that drew a bad copy are reported short, draw again and
// join a later batch while the next windows are in flight.  256 KiB slots at RS(3,2) so that many
// batches, and the retries among them, go round the slots.
void damaged(size_t d, size_t p, size_t chunk, size_t slot_bytes) {
    const Written w = write_files(d, p, chunk);
    ChunkStore store = w.store;
    uint64_t z = 0xC0FFEEull + d;
    size_t bad = 0, copies = 0;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts)
            for (size_t i = 0; i < d + p; ++i, ++copies)
                if (next(z) % 100 == 0) {
                    // a location may be shared by equal chunks (zero padding): then already done
                    (void)store.corrupt(part.chunk(i).locations.at(0), part.chunksize / 2);
                    ++bad;
                }
    CHECK(copies >= 1000 && bad >= copies / 200 && bad <= copies / 50);
    compare(w, store, 0, slot_bytes);
}

void damaged_rs32() { damaged(3, 2, size_t(1) << 12, size_t(256) << 10); }

void damaged_rs104() { damaged(10, 4, size_t(1) << 16, size_t(64) << 20); }

// Slots smaller than the largest parts: those parts take read_many's path window by window, the
// others still stream.
void small_slots() {
    const Written w = write_files(3, 2, size_t(1) << 16);
    compare(w, w.store, 0, size_t(128) << 10);
    ChunkStore erased = w.store;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts)  // zero padding may share a location: erased once
            (void)erased.erase(part.chunk(1).locations.at(0));
    compare(w, erased, 0, size_t(128) << 10);
}

// A part whose copies run out: read_many_stream throws what read_many throws, at either depth,
// and the thread's reader takes the next call.
void too_few() {
    const size_t d = 3, p = 2;
    const Written w = write_files(d, p, size_t(1) << 12);
    ChunkStore store = w.store;
    const FilePart& part = w.refs[1].parts.at(0);  // the 683-byte file
    for (size_t i = 0; i < p + 1; ++i) CHECK(store.erase(part.chunk(i + 1).locations.at(0)));
    const std::vector<const FileReference*> ptrs = w.ptrs();
    for (size_t depth : {size_t(1), size_t(3)}) {
        bool stream_threw = false, many_threw = false;
        try {
            FileReference::read_many_stream(ptrs, store, 0, 4, {}, depth);
        } catch (const ErasureError& e) {
            stream_threw = e.error() == Error::TooFewShardsPresent;
        }
        try {
            FileReference::read_many(ptrs, store, 0);
        } catch (const ErasureError& e) {
            many_threw = e.error() == Error::TooFewShardsPresent;
        }
        CHECK(stream_threw);
        CHECK(many_threw);
        compare(w, w.store, 0);  // after the failure
    }
    // a corrupted copy where no spare is left: verification fails, the copies run out
    ChunkStore bad = w.store;
    for (size_t i = 0; i < p; ++i) CHECK(bad.erase(part.chunk(i).locations.at(0)));
    CHECK(bad.corrupt(part.chunk(p).locations.at(0), 0));
    bool threw = false;
    try {
        FileReference::read_many_stream(ptrs, bad, 0, 4, {}, 2);
    } catch (const ErasureError& e) {
        threw = e.error() == Error::TooFewShardsPresent;
    }
    CHECK(threw);
}

// RS(4,9) is outside the reader (p > 8): read_many's path, the same bytes.
void refused_shape() {
    const size_t d = 4, p = 9;
    Written w;
    for (size_t n : {size_t(1), size_t(683), size_t(20480), size_t(300000)})
        w.files.push_back(random_bytes(n, n));
    std::vector<std::pair<const uint8_t*, size_t>> views;
    for (const Bytes& f : w.files) views.emplace_back(f.data(), f.size());
    w.refs = FileWriteBuilder().chunk_size(size_t(1) << 12).data_chunks(d).parity_chunks(p)
                 .write_many(views, w.store);
    compare(w, w.store, 0);
    ChunkStore erased = w.store;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts) CHECK(erased.erase(part.chunk(0).locations.at(0)));
    compare(w, erased, 0);
}

// release_thread_buffers hands the thread's reader back; the next call makes it again.
void released() {
    const Written w = write_files(3, 2, size_t(1) << 12);
    compare(w, w.store, 0);
    release_thread_buffers();
    compare(w, w.store, 0);
    release_thread_buffers();
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"rs32", rs32},
    {"rs104", rs104},
    {"mixed_batch", mixed_batch},
    {"damaged_rs32", damaged_rs32},
    {"damaged_rs104", damaged_rs104},
    {"small_slots", small_slots},
    {"too_few", too_few},
    {"refused_shape", refused_shape},
    {"released", released},
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
