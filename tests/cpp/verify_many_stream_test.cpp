// verify_many_stream_test.cpp — FileReference::verify_many_stream against verify_many, report for
// report, on the real engine.
//
// The stream sends every copy the skeleton rule leaves to be checked through the scrub pipeline
// (cec_scrub_pipeline_*) as segments, its SHA-256 chain resumed from a record on the device; the
// reports must be what verify_many gives from one cec_parts_verify call per window.  Files: sizes
// 0, 1, 683, 20480, 100007 and 2 * d * chunk + 5, written with write_many.  Stores: intact; one
// copy of every part missing; and, in every part, a corrupted copy, a copy of the wrong size and a
// chunk with two locations whose first copy is bad.  Settings: segments of 64 up to more than a
// chunk, slots of one segment up to ample, depth 1 to 3, max_open 1, a few and the default.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_verify_many_stream.py runs one process per case, so a crash names its case).
#include <cstdio>
#include <cstring>
#include <map>
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

struct Written {
    std::vector<Bytes> files;
    std::vector<FileReference> refs;
    ChunkStore store;
};

Written write_files(size_t d, size_t p, size_t chunk) {
    Written w;
    const size_t sizes[] = {0, 1, 683, 20480, 100007, 2 * d * chunk + 5};
    uint64_t seed = 1;
    for (size_t size : sizes) w.files.push_back(random_bytes(size, seed++));
    std::vector<std::pair<const uint8_t*, size_t>> views;
    for (const Bytes& f : w.files) views.emplace_back(f.data(), f.size());
    w.refs = FileWriteBuilder().chunk_size(chunk).data_chunks(d).parity_chunks(p).write_many(
        views, w.store);
    return w;
}

std::map<Location, size_t> location_refs(const std::vector<FileReference>& refs) {
    std::map<Location, size_t> n;
    for (const FileReference& r : refs)
        for (const FilePart& part : r.parts)
            for (size_t i = 0; i < part.data.size() + part.parity.size(); ++i)
                for (const Location& loc : part.chunk(i).locations) ++n[loc];
    return n;
}

constexpr size_t kNone = size_t(-1);

// The first chunk of `part`, other than skip_a and skip_b, whose one location no other chunk
// lists: damage there is this part's alone.  kNone when there is none.
size_t find_own_chunk(const std::map<Location, size_t>& refs, const FilePart& part,
                      size_t skip_a = kNone, size_t skip_b = kNone) {
    for (size_t i = 0; i < part.data.size() + part.parity.size(); ++i)
        if (i != skip_a && i != skip_b && part.chunk(i).locations.size() == 1 &&
            refs.at(part.chunk(i).locations[0]) == 1)
            return i;
    return kNone;
}

std::vector<const FileReference*> const_ptrs(const std::vector<FileReference>& refs) {
    std::vector<const FileReference*> v;
    for (const FileReference& r : refs) v.push_back(&r);
    return v;
}

bool same_report(const PartReport& a, const PartReport& b) {
    return a.locations == b.locations && a.chunks == b.chunks &&
           a.new_locations == b.new_locations && a.write_error == b.write_error;
}

struct Setting {
    size_t segment, slot, depth, max_open;
};

// verify_many_stream under every setting against verify_many; returns verify_many's reports.
std::vector<std::vector<PartReport>> compare(const std::vector<FileReference>& refs,
                                             const ChunkStore& store, size_t chunk) {
    const auto want = FileReference::verify_many(const_ptrs(refs), store);
    const Setting settings[] = {
        {256, 256, 1, 1},                     // a slot of one segment, one copy under way
        {64, 4096, 2, 3},                     // dozens of batches a copy
        {192, 1000, 3, 1},                    // a slot that is no multiple of the segment
        {1024, 1 << 16, 3, 0},                // the default number of open copies
        {(chunk * 2 + 63) / 64 * 64, size_t(1) << 20, 2, 0},  // every copy whole
        {16384, size_t(64) << 20, 3, 0},      // the defaults
    };
    for (const Setting& s : settings) {
        const auto got = FileReference::verify_many_stream(const_ptrs(refs), store, s.segment,
                                                           s.slot, s.depth, s.max_open);
        CHECK(got.size() == want.size());
        for (size_t f = 0; f < want.size() && f < got.size(); ++f) {
            CHECK(got[f].size() == want[f].size());
            for (size_t k = 0; k < want[f].size() && k < got[f].size(); ++k)
                if (!same_report(got[f][k], want[f][k])) {
                    std::fprintf(stderr, "  segment %zu slot %zu depth %zu max_open %zu: file %zu "
                                 "part %zu differs\n", s.segment, s.slot, s.depth, s.max_open, f, k);
                    ++g_failures;
                }
        }
    }
    return want;
}

size_t count_parts(const std::vector<std::vector<PartReport>>& reports, bool ideal) {
    size_t n = 0;
    for (const auto& file : reports)
        for (const PartReport& rep : file) n += rep.is_ideal() == ideal;
    return n;
}

void stores(size_t d, size_t p, size_t chunk) {
    const Written w = write_files(d, p, chunk);
    const auto refs = location_refs(w.refs);
    size_t n_parts = 0;
    for (const FileReference& r : w.refs) n_parts += r.parts.size();
    CHECK(n_parts >= 8);
    CHECK(count_parts(compare(w.refs, w.store, chunk), true) == n_parts);

    ChunkStore erased = w.store;  // one copy of every part does not read
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts) {
            const size_t a = find_own_chunk(refs, part);
            CHECK(a != kNone);
            if (a != kNone) CHECK(erased.erase(part.chunk(a).locations[0]));
        }
    auto reports = compare(w.refs, erased, chunk);
    CHECK(count_parts(reports, false) == n_parts);

    ChunkStore damaged = w.store;
    std::vector<FileReference> listed = w.refs;  // with the replicas' locations
    size_t replica = 0, shortened = 0;
    for (FileReference& r : listed)
        for (FilePart& part : r.parts) {
            const size_t a = find_own_chunk(refs, part);
            CHECK(a != kNone);
            if (a == kNone) continue;
            // the last byte: with chunks longer than a segment, in the copy's last segment
            CHECK(damaged.corrupt(part.chunk(a).locations[0], part.chunksize - 1));
            const size_t b = find_own_chunk(refs, part, a);
            if (b == kNone) continue;
            const Bytes* whole = damaged.find(part.chunk(b).locations[0]);
            damaged.put(part.chunk(b).locations[0], Bytes(whole->begin(), whole->end() - 1));
            ++shortened;
            // a replica listed first, with a flipped bit in its middle byte (a middle segment
            // of a long copy); the written copy behind it is good
            const size_t c = find_own_chunk(refs, part, a, b);
            if (c == kNone) continue;
            Chunk& ch = part.chunk_mut(c);
            Bytes bad = *damaged.find(ch.locations[0]);
            bad[bad.size() / 2] ^= 0x01;
            const Location loc = "replica-" + std::to_string(replica++);
            damaged.put(loc, bad);
            ch.locations.insert(ch.locations.begin(), loc);
        }
    CHECK(replica + 2 >= n_parts && shortened + 2 >= n_parts);
    reports = compare(listed, damaged, chunk);
    CHECK(count_parts(reports, false) == n_parts);
    size_t first_bad = 0, invalid = 0;
    for (const auto& file : reports)
        for (const PartReport& rep : file) {
            invalid += rep.invalid_locations();
            for (size_t i = 0; i < rep.locations.size(); ++i)
                first_bad += rep.locations[i].size() == 2 &&
                             rep.locations[i][0] == LocationIntegrity::Invalid &&
                             rep.locations[i][1] == LocationIntegrity::Valid;
        }
    CHECK(first_bad == replica && invalid == n_parts + shortened + replica);
}

// The planner's own refusals reach the caller, and leave the pipeline usable.
void refusals() {
    const Written w = write_files(3, 2, 4096);
    const auto ptrs = const_ptrs(w.refs);
    auto throws = [&](size_t segment, size_t slot) {
        try {
            (void)FileReference::verify_many_stream(ptrs, w.store, segment, slot, 2, 0);
        } catch (const std::invalid_argument&) {
            return true;
        }
        return false;
    };
    CHECK(throws(100, 1 << 16));  // no multiple of 64
    CHECK(throws(0, 1 << 16));
    CHECK(throws(1024, 512));     // a slot below one segment
    const auto want = FileReference::verify_many(ptrs, w.store);
    const auto got = FileReference::verify_many_stream(ptrs, w.store, 1024, 1 << 16, 2, 0);
    CHECK(got.size() == want.size());
    for (size_t f = 0; f < want.size() && f < got.size(); ++f)
        for (size_t k = 0; k < want[f].size() && k < got[f].size(); ++k)
            CHECK(same_report(got[f][k], want[f][k]));
    // no files, and files without parts
    CHECK(FileReference::verify_many_stream({}, w.store).empty());
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"stream_rs32", [] { stores(3, 2, 4096); }},
    {"stream_rs104", [] { stores(10, 4, 1000); }},
    {"refusals", refusals},
};

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "--list") == 0) {
        for (const Case& c : kCases) std::printf("%s\n", c.name);
        return 0;
    }
    for (const Case& c : kCases) {
        if (argc == 2 && std::strcmp(argv[1], c.name) != 0) continue;
        std::printf("%s ... ", c.name);
        std::fflush(stdout);
        const int before = g_failures;
        try {
            c.fn();
        } catch (const std::exception& e) {
            std::fprintf(stderr, "  exception: %s\n", e.what());
            ++g_failures;
        }
        std::printf("%s\n", g_failures == before ? "ok" : "FAILED");
    }
    return g_failures ? 1 : 0;
}
