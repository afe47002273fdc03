// write_many_stream_test.cpp — FileWriteBuilder::write_many_stream against write(), file by file.
//
// write_many_stream sends every part that is not a full part of a batched file through the
// calling thread's ragged write pipeline (cec_parts_pipeline_*), a slot's batch at a time with
// the other slots in flight.  The result must be what write() gives for each file on its own:
// the same FileReference (parts, chunksize, digests, locations, length), the same stored chunks,
// and the chunks handed to the store in file, part, chunk order.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_write_many_stream.py runs one process per case, so a crash names its case).
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

// Files of 1 B to ~300 KiB, an empty one among them, ~5 MiB in all: with 1 MiB slots and two of
// them every slot is used several times.
std::vector<Bytes> small_files(size_t count) {
    std::vector<Bytes> files;
    uint64_t z = 12345;
    for (size_t f = 0; f < count; ++f) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        const size_t size = f == 7 ? 0 : f % 9 == 0 ? 1 + (z >> 33) % 16 : 1 + (z >> 33) % (300u << 10);
        files.push_back(random_bytes(size, f + 1));
    }
    return files;
}

void slots_reused() {
    const std::vector<Bytes> files = small_files(36);
    compare(FileWriteBuilder().chunk_size(size_t(1) << 17).data_chunks(3).parity_chunks(2)
                .many_slots(size_t(1) << 20, 2), files);
    compare(FileWriteBuilder().chunk_size(size_t(1) << 16).data_chunks(10).parity_chunks(4)
                .many_slots(size_t(1) << 20, 2), files);
}

// A file with three full parts and a tail between small files, batch() set: its full parts go
// through the batched full-parts path after everything before them has reached the store.
void full_parts_in_the_middle() {
    for (const auto& shape : {std::pair<size_t, size_t>{3, 2}, {10, 4}}) {
        const size_t d = shape.first, chunk = size_t(1) << 14;
        std::vector<Bytes> files = small_files(12);
        files.insert(files.begin() + 5, random_bytes(3 * d * chunk + 4321, 77));
        files.insert(files.begin() + 9, random_bytes(2 * d * chunk, 78));
        compare(FileWriteBuilder().chunk_size(chunk).data_chunks(d).parity_chunks(shape.second)
                    .batch(8, 3).many_slots(size_t(1) << 20, 2), files);
    }
}

void empty_files() {
    compare(FileWriteBuilder().data_chunks(3).parity_chunks(2).many_slots(size_t(1) << 20, 2),
            {Bytes()});
    compare(FileWriteBuilder().data_chunks(3).parity_chunks(2).many_slots(size_t(1) << 20, 2),
            {Bytes(), random_bytes(683, 5), Bytes()});
    compare(FileWriteBuilder().data_chunks(3).parity_chunks(2), {});
}

// many_slots below one part: the slot is raised to d * stride(chunk_size), which a full part
// fills exactly; parts of that size alternate with small ones, with three slots and with one.
void part_equal_to_the_slot_minimum() {
    const size_t d = 3, chunk = (size_t(1) << 16) + 5;  // stride 65552
    std::vector<Bytes> files;
    for (int r = 0; r < 3; ++r) {
        files.push_back(random_bytes(d * chunk, 90 + r));       // one full part, alone in a slot
        files.push_back(random_bytes(1000 + r, 95 + r));
        files.push_back(random_bytes(d * chunk + 17, 99 + r));  // a full part and a 17-byte tail
    }
    for (size_t depth : {size_t(3), size_t(1)})
        compare(FileWriteBuilder().chunk_size(chunk).data_chunks(d).parity_chunks(2)
                    .many_slots(16, depth), files);
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"slots_reused", slots_reused},
    {"full_parts_in_the_middle", full_parts_in_the_middle},
    {"empty_files", empty_files},
    {"part_equal_to_the_slot_minimum", part_equal_to_the_slot_minimum},
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
