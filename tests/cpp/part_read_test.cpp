// part_read_test.cpp — FilePart::read_coalesced against read_with_context, concurrent readers.
//
// 16 threads, each reading its own FilePart of a different size (whole small files written as one
// part each, chunk sizes from 3 bytes to 64 KiB and more, most of them no multiple of 16), released
// together so their cec_part_read calls meet in the coalescer.  Every case reads three kinds of
// store: intact, the first data chunk of every part erased (rebuilt from parity), and that chunk
// with two locations, [bad, good] (the first copy fails verification, the part is reported short
// and the next round loads the good copy beside the chunks already verified).  The result must be
// read_with_context's, and the file's bytes.  A part without d good chunks throws
// TooFewShardsPresent from both.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_part_read_cpp.py runs one process per case, so a crash names its case).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "chunky_ec.hpp"

using namespace chunky_ec;

namespace {

std::atomic<int> g_failures{0};

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

constexpr size_t kThreads = 16;

// File k of a shape with d data chunks: one part whose chunk size is sizes[k] (ceil(len / d)).
size_t file_len(size_t d, size_t k) {
    const size_t chunk_sizes[kThreads] = {3,    15,   16,   17,    255,   256,   1000,  4096,
                                          4099, 9999, 16384, 30001, 50000, 65536, 65539, 70001};
    return d * chunk_sizes[k] - (k % d);  // a short last data chunk where k % d != 0
}

struct Written {
    std::vector<Bytes> files;
    std::vector<FileReference> refs;
    ChunkStore store;
};

Written write_files(size_t d, size_t p) {
    Written w;
    const FileWriteBuilder b =
        FileWriteBuilder().chunk_size(size_t(1) << 20).data_chunks(d).parity_chunks(p);
    for (size_t k = 0; k < kThreads; ++k) {
        w.files.push_back(random_bytes(file_len(d, k), 100 * d + k));
        w.refs.push_back(b.write(w.files.back(), w.store));
        CHECK(w.refs.back().parts.size() == 1);
    }
    return w;
}

// Every part read by its own thread, all released together; against read_with_context (read one
// by one) and the file's bytes.
void compare(const Written& w, const std::vector<FilePart>& parts, const ChunkStore& store) {
    std::vector<Bytes> got(kThreads);
    std::vector<std::string> err(kThreads);
    std::atomic<size_t> ready{0};
    std::vector<std::thread> th;
    for (size_t k = 0; k < kThreads; ++k)
        th.emplace_back([&, k] {
            ++ready;
            while (ready.load() < kThreads) std::this_thread::yield();
            try {
                got[k] = parts[k].read_coalesced(store);
            } catch (const std::exception& e) {
                err[k] = e.what();
            }
        });
    for (std::thread& t : th) t.join();
    for (size_t k = 0; k < kThreads; ++k) {
        CHECK(err[k].empty());
        const Bytes want = parts[k].read_with_context(store);
        CHECK(got[k] == want);
        CHECK(got[k].size() >= w.files[k].size() &&
              std::equal(w.files[k].begin(), w.files[k].end(), got[k].begin()));
    }
}

void three_stores(size_t d, size_t p) {
    const Written w = write_files(d, p);
    std::vector<FilePart> parts;
    for (const FileReference& r : w.refs) parts.push_back(r.parts.at(0));
    uint64_t calls0 = 0, launches0 = 0, calls1 = 0, launches1 = 0;
    cec_coalesce_detail(nullptr, &calls0, &launches0);
    compare(w, parts, w.store);
    cec_coalesce_detail(nullptr, &calls1, &launches1);
    CHECK(calls1 - calls0 == kThreads);  // intact: one round per part
    CHECK(launches1 - launches0 >= 1 && launches1 - launches0 <= kThreads);

    ChunkStore erased = w.store, bad_good = w.store;
    std::vector<FilePart> two = parts;  // chunk 0 of every part at [bad, good]
    for (size_t k = 0; k < kThreads; ++k) {
        const Location loc = parts[k].chunk(0).locations.at(0);
        CHECK(erased.erase(loc));
        Bytes bad = *w.store.find(loc);
        bad[bad.size() - 1] ^= 0x01;
        const Location bad_loc = "stale-" + loc;
        bad_good.put(bad_loc, bad);
        two[k].chunk_mut(0).locations = {bad_loc, loc};
    }
    compare(w, parts, erased);
    compare(w, two, bad_good);
}

void rs32() { three_stores(3, 2); }
void rs104() { three_stores(10, 4); }

// p + 1 chunks of a part erased: both readers throw TooFewShardsPresent; the other parts, read at
// the same time, are not disturbed.
void too_few() {
    const size_t d = 3, p = 2;
    const Written w = write_files(d, p);
    ChunkStore store = w.store;
    const FilePart& part = w.refs[6].parts.at(0);
    for (size_t i = 0; i < p + 1; ++i) CHECK(store.erase(part.chunk(i + 1).locations.at(0)));
    std::vector<Bytes> got(kThreads);
    std::vector<int> threw(kThreads, 0);
    std::vector<std::thread> th;
    for (size_t k = 0; k < kThreads; ++k)
        th.emplace_back([&, k] {
            try {
                got[k] = w.refs[k].parts.at(0).read_coalesced(store);
            } catch (const ErasureError& e) {
                threw[k] = e.error() == Error::TooFewShardsPresent ? 1 : 2;
            }
        });
    for (std::thread& t : th) t.join();
    for (size_t k = 0; k < kThreads; ++k) {
        CHECK(threw[k] == (k == 6 ? 1 : 0));
        if (k != 6) CHECK(got[k] == w.refs[k].parts.at(0).read_with_context(store));
    }
    bool one_threw = false;
    try {
        part.read_with_context(store);
    } catch (const ErasureError& e) {
        one_threw = e.error() == Error::TooFewShardsPresent;
    }
    CHECK(one_threw);
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"rs32", rs32},
    {"rs104", rs104},
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
