// check_many_test.cpp — FileReference::verify_many / resilver_many against verify() / resilver(),
// file by file.
//
// The two calls gather every part that is not in a batched run of one shape -- whole small
// files, short last parts, every part when parts_per_batch is 0 -- into ragged batches
// (cec_parts_verify, cec_parts_read); the reports, the files' location lists and the store must
// be what verify() / resilver() give for each file on its own.  Files: those of
// write_many_test.cpp (sizes 0, 1, 683, 20480, 3*2^20 + 7 and 2*d*chunk + 5), written with
// write_many.  A location that is damaged is always one that a single chunk lists (the program
// checks it), except in shared_location, which is about the other kind.
//
// Runs on a GPU.  `--list` prints the case names; a name runs that case alone
// (tests/test_gpu_check_many.py runs one process per case, so a crash names its case).
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

Written write_files(const std::vector<Bytes>& files, size_t d, size_t p, size_t chunk) {
    Written w;
    w.files = files;
    std::vector<std::pair<const uint8_t*, size_t>> views;
    for (const Bytes& f : w.files) views.emplace_back(f.data(), f.size());
    w.refs = FileWriteBuilder().chunk_size(chunk).data_chunks(d).parity_chunks(p).write_many(
        views, w.store);
    return w;
}

// How many chunks of these files list each location.
std::map<Location, size_t> location_refs(const std::vector<FileReference>& refs) {
    std::map<Location, size_t> n;
    for (const FileReference& r : refs)
        for (const FilePart& part : r.parts)
            for (size_t i = 0; i < part.data.size() + part.parity.size(); ++i)
                for (const Location& loc : part.chunk(i).locations) ++n[loc];
    return n;
}

constexpr size_t kNone = size_t(-1);

// The first chunk among [from, to) of `part`, other than skip_a and skip_b, whose one location
// no other chunk lists: damage there is this part's alone.  kNone when there is none.
size_t find_own_chunk(const std::map<Location, size_t>& refs, const FilePart& part, size_t from,
                      size_t to, size_t skip_a = kNone, size_t skip_b = kNone) {
    for (size_t i = from; i < to; ++i)
        if (i != skip_a && i != skip_b && part.chunk(i).locations.size() == 1 &&
            refs.at(part.chunk(i).locations[0]) == 1)
            return i;
    return kNone;
}

// The same where the case needs one: a part without is a failure.
size_t own_chunk(const std::map<Location, size_t>& refs, const FilePart& part, size_t from,
                 size_t to, size_t skip = kNone) {
    const size_t i = find_own_chunk(refs, part, from, to, skip);
    const bool has_a_chunk_of_its_own = i != kNone;
    CHECK(has_a_chunk_of_its_own);
    return has_a_chunk_of_its_own ? i : from;
}

std::vector<const FileReference*> const_ptrs(const std::vector<FileReference>& refs) {
    std::vector<const FileReference*> v;
    for (const FileReference& r : refs) v.push_back(&r);
    return v;
}

std::vector<FileReference*> mut_ptrs(std::vector<FileReference>& refs) {
    std::vector<FileReference*> v;
    for (FileReference& r : refs) v.push_back(&r);
    return v;
}

bool same_report(const PartReport& a, const PartReport& b) {
    return a.locations == b.locations && a.chunks == b.chunks &&
           a.new_locations == b.new_locations && a.write_error == b.write_error;
}

// verify_many over `refs` against verify() file by file; returns verify_many's reports.
std::vector<std::vector<PartReport>> compare_verify(const std::vector<FileReference>& refs,
                                                    const ChunkStore& store, size_t ppb) {
    auto got = FileReference::verify_many(const_ptrs(refs), store, ppb);
    CHECK(got.size() == refs.size());
    if (got.size() != refs.size()) return got;
    for (size_t f = 0; f < refs.size(); ++f) {
        const std::vector<PartReport> one = refs[f].verify(store, ppb);
        CHECK(got[f].size() == one.size() && one.size() == refs[f].parts.size());
        for (size_t k = 0; k < one.size() && k < got[f].size(); ++k)
            CHECK(same_report(got[f][k], one[k]));
    }
    return got;
}

size_t count_parts(const std::vector<std::vector<PartReport>>& reports, bool ideal) {
    size_t n = 0;
    for (const auto& file : reports)
        for (const PartReport& rep : file) n += rep.is_ideal() == ideal;
    return n;
}

// Every part ideal under verify_many, and read_many gives the files' bytes.
void check_whole(const std::vector<FileReference>& refs, const std::vector<Bytes>& files,
                 const ChunkStore& store, size_t ppb) {
    CHECK(count_parts(compare_verify(refs, store, ppb), false) == 0);
    const std::vector<Bytes> got = FileReference::read_many(const_ptrs(refs), store, ppb);
    CHECK(got == files);
}

// The store intact; with one chunk of every part erased; with a corrupted copy, a copy of the
// wrong size and a two-location chunk whose first copy is bad in every part.
void verify_stores(size_t d, size_t p, size_t chunk, size_t ppb) {
    const Written w = write_files(make_files(d, chunk), d, p, chunk);
    const size_t t = d + p;
    const auto refs = location_refs(w.refs);
    size_t n_parts = 0;
    for (const FileReference& r : w.refs) n_parts += r.parts.size();
    CHECK(n_parts >= 8);
    CHECK(count_parts(compare_verify(w.refs, w.store, ppb), true) == n_parts);

    ChunkStore erased = w.store;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts)
            CHECK(erased.erase(part.chunk(own_chunk(refs, part, 0, t)).locations[0]));
    auto reports = compare_verify(w.refs, erased, ppb);
    CHECK(count_parts(reports, false) == n_parts);
    for (const auto& file : reports)
        for (const PartReport& rep : file) CHECK(rep.unavailable_locations() == 1);

    ChunkStore damaged = w.store;
    std::vector<FileReference> listed = w.refs;  // with the replicas' locations
    size_t replica = 0, shortened = 0;
    for (FileReference& r : listed)
        for (FilePart& part : r.parts) {
            // (a part of one-byte chunks may have fewer than three chunks of its own: its zero
            // padding, and a parity byte that equals a data byte, share their locations)
            const size_t a = own_chunk(refs, part, 0, t), b = find_own_chunk(refs, part, 0, t, a);
            CHECK(damaged.corrupt(part.chunk(a).locations[0], part.chunksize - 1));
            if (b == kNone) continue;
            const Bytes* whole = damaged.find(part.chunk(b).locations[0]);
            damaged.put(part.chunk(b).locations[0], Bytes(whole->begin(), whole->end() - 1));
            ++shortened;
            // a replica listed first, with a flipped bit; the written copy behind it is good
            const size_t c = find_own_chunk(refs, part, 0, t, a, b);
            if (c == kNone) continue;
            Chunk& ch = part.chunk_mut(c);
            Bytes bad = *damaged.find(ch.locations[0]);
            bad[0] ^= 0x01;
            const Location loc = "replica-" + std::to_string(replica++);
            damaged.put(loc, bad);
            ch.locations.insert(ch.locations.begin(), loc);
        }
    CHECK(replica + 2 >= n_parts && shortened + 2 >= n_parts);
    reports = compare_verify(listed, damaged, ppb);
    CHECK(count_parts(reports, false) == n_parts);
    size_t first_bad = 0, invalid = 0;
    for (const auto& file : reports)
        for (const PartReport& rep : file) {
            CHECK(rep.invalid_locations() >= 1 && rep.unavailable_locations() == 0);
            invalid += rep.invalid_locations();
            for (size_t i = 0; i < rep.locations.size(); ++i)
                first_bad += rep.locations[i].size() == 2 &&
                             rep.locations[i][0] == LocationIntegrity::Invalid &&
                             rep.locations[i][1] == LocationIntegrity::Valid &&
                             rep.chunks[i] == LocationIntegrity::Valid;
        }
    CHECK(first_bad == replica && invalid == n_parts + shortened + replica);
}

// resilver_many on one copy of (refs, store) against resilver() file by file on another: the
// reports, the files' location lists, the stores' sizes.  Returns resilver_many's side.
struct Resilvered {
    std::vector<FileReference> refs;
    ChunkStore store;
    std::vector<std::vector<PartReport>> reports;
};

Resilvered compare_resilver(const std::vector<FileReference>& refs, const ChunkStore& store,
                            size_t ppb) {
    Resilvered many{refs, store, {}};
    std::vector<FileReference> one_refs = refs;
    ChunkStore one_store = store;
    many.reports = FileReference::resilver_many(mut_ptrs(many.refs), many.store, ppb);
    CHECK(many.reports.size() == refs.size());
    if (many.reports.size() != refs.size()) return many;
    for (size_t f = 0; f < refs.size(); ++f) {
        const std::vector<PartReport> one = one_refs[f].resilver(one_store, ppb);
        CHECK(many.reports[f].size() == one.size());
        for (size_t k = 0; k < one.size() && k < many.reports[f].size(); ++k) {
            CHECK(same_report(many.reports[f][k], one[k]));
            const FilePart &a = many.refs[f].parts[k], &b = one_refs[f].parts[k];
            for (size_t i = 0; i < a.data.size() + a.parity.size(); ++i) {
                CHECK(a.chunk(i).locations == b.chunk(i).locations);
                for (const Location& loc : a.chunk(i).locations) {
                    const Bytes *x = many.store.find(loc), *y = one_store.find(loc);
                    CHECK((!x && !y) || (x && y && *x == *y));
                }
            }
        }
    }
    CHECK(many.store.size() == one_store.size());
    return many;
}

// One data and one parity chunk of every part erased (of those with a location of their own: a
// part of one-byte chunks may lack one of the two), and the lone copy of one more chunk corrupted
// in one part (where p leaves room for a third lost chunk; else that part's parity chunk is
// corrupted instead of erased).  Returns the number of chunks damaged.
size_t damage_for_resilver(const Written& w, size_t d, size_t p, ChunkStore& store) {
    const size_t t = d + p;
    const auto refs = location_refs(w.refs);
    bool corrupted = false;
    size_t damaged = 0, n_parts = 0;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts) {
            ++n_parts;
            const size_t a = find_own_chunk(refs, part, 0, d), b = find_own_chunk(refs, part, d, t);
            CHECK(a != kNone || b != kNone);
            if (a != kNone) CHECK(store.erase(part.chunk(a).locations[0]));
            damaged += (a != kNone) + (b != kNone);
            if (b == kNone) continue;
            const bool here = !corrupted && part.chunksize > 100;
            damaged += here && p >= 3;
            if (here && p < 3) {
                CHECK(store.corrupt(part.chunk(b).locations[0], 0));
            } else {
                CHECK(store.erase(part.chunk(b).locations[0]));
                if (here)
                    CHECK(store.corrupt(part.chunk(own_chunk(refs, part, d, t, b)).locations[0], 0));
            }
            corrupted = corrupted || here;
        }
    CHECK(corrupted && damaged + 2 >= 2 * n_parts + (p >= 3));
    return damaged;
}

void resilver_case(size_t d, size_t p, size_t chunk, size_t ppb) {
    const Written w = write_files(make_files(d, chunk), d, p, chunk);
    ChunkStore store = w.store;
    const size_t damaged = damage_for_resilver(w, d, p, store);
    const Resilvered r = compare_resilver(w.refs, store, ppb);
    size_t invalid = 0, rebuilt = 0;
    for (const auto& file : r.reports)
        for (const PartReport& rep : file) {
            CHECK(!rep.write_error && rep.is_ideal());
            CHECK(rep.count(LocationIntegrity::Resilvered) == rep.new_locations.size());
            CHECK(rep.new_locations.size() >= 1);
            rebuilt += rep.new_locations.size();
            invalid += rep.invalid_locations();
        }
    CHECK(invalid == 1 && rebuilt == damaged);
    check_whole(r.refs, w.files, r.store, ppb);
}

void verify_rs32() { verify_stores(3, 2, size_t(1) << 10, 0); }
void verify_rs104() { verify_stores(10, 4, size_t(1) << 16, 0); }
void resilver_rs32() { resilver_case(3, 2, size_t(1) << 10, 0); }
void resilver_rs104() { resilver_case(10, 4, size_t(1) << 16, 0); }

// p + 1 chunks of one part gone: that part gets write_error, the rest are resilvered.
void too_few() {
    const size_t d = 3, p = 2, t = d + p;
    const Written w = write_files(make_files(d, size_t(1) << 10), d, p, size_t(1) << 10);
    const auto refs = location_refs(w.refs);
    ChunkStore store = w.store;
    const FilePart& lost = w.refs[2].parts.at(0);  // the 683-byte file
    for (size_t i = 1; i < p + 2; ++i) {
        CHECK(refs.at(lost.chunk(i).locations.at(0)) == 1);
        CHECK(store.erase(lost.chunk(i).locations[0]));
    }
    size_t n_parts = 0;
    for (const FileReference& r : w.refs)
        for (const FilePart& part : r.parts) {
            ++n_parts;
            if (&part != &lost) CHECK(store.erase(part.chunk(own_chunk(refs, part, 0, t)).locations[0]));
        }
    for (size_t ppb : {size_t(0), size_t(8)}) {
        const Resilvered r = compare_resilver(w.refs, store, ppb);
        for (size_t f = 0; f < r.reports.size(); ++f)
            for (size_t k = 0; k < r.reports[f].size(); ++k) {
                const PartReport& rep = r.reports[f][k];
                if (f == 2) {
                    CHECK(rep.write_error && *rep.write_error == Error::TooFewShardsPresent);
                    CHECK(rep.new_locations.empty());
                } else {
                    CHECK(!rep.write_error && rep.is_ideal() && rep.new_locations.size() == 1);
                }
            }
        const auto after = compare_verify(r.refs, r.store, ppb);
        CHECK(count_parts(after, false) == 1 && count_parts(after, true) == n_parts - 1);
    }
}

// parts_per_batch = 8: the runs of two or more parts of one shape go through check_run, every
// other part through the ragged calls, in one call.
void mixed_batch() {
    verify_stores(3, 2, size_t(1) << 10, 8);
    resilver_case(3, 2, size_t(1) << 10, 8);
    verify_stores(10, 4, size_t(1) << 16, 8);
    resilver_case(10, 4, size_t(1) << 16, 8);
}

// RS(3,2) and RS(10,4) files in one call: one verify window for both, a resilver window each.
void mixed_shapes() {
    const Written a = write_files(make_files(3, size_t(1) << 10), 3, 2, size_t(1) << 10);
    const Written b = write_files(make_files(10, size_t(1) << 16), 10, 4, size_t(1) << 16);
    std::vector<FileReference> refs;
    std::vector<Bytes> files;
    ChunkStore store = a.store;
    for (size_t f = 0; f < a.refs.size(); ++f) {  // interleaved
        refs.push_back(a.refs[f]);
        refs.push_back(b.refs[f]);
        files.push_back(a.files[f]);
        files.push_back(b.files[f]);
    }
    for (const FileReference& r : b.refs)
        for (const FilePart& part : r.parts)
            for (size_t i = 0; i < 14; ++i)
                store.put(part.chunk(i).locations.at(0), *b.store.find(part.chunk(i).locations[0]));
    const auto lrefs = location_refs(refs);
    // a data chunk erased and a parity chunk corrupted in every part (where it has one of its
    // own: the one-byte file is the same byte under both shapes)
    size_t n_parts = 0, damaged = 0;
    for (const FileReference& r : refs)
        for (const FilePart& part : r.parts) {
            const size_t d = part.data.size(), t = d + part.parity.size();
            const size_t a = find_own_chunk(lrefs, part, 0, d), b = find_own_chunk(lrefs, part, d, t);
            CHECK(a != kNone || b != kNone);
            if (a != kNone) CHECK(store.erase(part.chunk(a).locations[0]));
            if (b != kNone) CHECK(store.corrupt(part.chunk(b).locations[0], 0));
            damaged += (a != kNone) + (b != kNone);
            ++n_parts;
        }
    CHECK(damaged + 4 >= 2 * n_parts);
    for (size_t ppb : {size_t(0), size_t(8)}) {
        CHECK(count_parts(compare_verify(refs, store, ppb), false) == n_parts);
        const Resilvered r = compare_resilver(refs, store, ppb);
        size_t rebuilt = 0;
        for (const auto& file : r.reports)
            for (const PartReport& rep : file) {
                CHECK(rep.is_ideal() && !rep.new_locations.empty());
                rebuilt += rep.new_locations.size();
            }
        CHECK(rebuilt == damaged);
        check_whole(r.refs, files, r.store, ppb);
    }
}

// Two files whose first data chunk is the same 1024 bytes, stored once, and erased: both parts
// are judged against the store as it was loaded, both report the chunk Resilvered, it is written
// twice with the same bytes, and the store ends up whole.
void shared_location() {
    const size_t d = 3, p = 2, chunk = size_t(1) << 10;
    std::vector<Bytes> files = {random_bytes(d * chunk, 11), random_bytes(d * chunk, 12)};
    std::copy(files[0].begin(), files[0].begin() + chunk, files[1].begin());
    const Written w = write_files(files, d, p, chunk);
    CHECK(w.refs[0].parts.size() == 1 && w.refs[1].parts.size() == 1);
    const Location shared = w.refs[0].parts[0].chunk(0).locations.at(0);
    CHECK(w.refs[1].parts[0].chunk(0).locations.at(0) == shared);
    CHECK(w.store.size() == 2 * (d + p) - 1);
    Resilvered r{w.refs, w.store, {}};
    CHECK(r.store.erase(shared));
    std::vector<Location> written;
    r.store.log_writes(&written);
    r.reports = FileReference::resilver_many(mut_ptrs(r.refs), r.store);
    r.store.log_writes(nullptr);
    CHECK(written == std::vector<Location>(2, shared));
    CHECK(r.store.size() == w.store.size());
    CHECK(*r.store.find(shared) == *w.store.find(shared));
    for (size_t f = 0; f < 2; ++f) {
        const PartReport& rep = r.reports.at(f).at(0);
        CHECK(!rep.write_error && rep.is_ideal());
        CHECK(rep.chunks[0] == LocationIntegrity::Resilvered);
        CHECK(rep.count(LocationIntegrity::Resilvered) == 1);
        CHECK(rep.new_locations == std::vector<Location>(1, shared));
        CHECK(r.refs[f].parts[0].chunk(0).locations == std::vector<Location>(2, shared));
    }
    check_whole(r.refs, w.files, r.store, 0);
}

struct Case {
    const char* name;
    void (*fn)();
};

const Case kCases[] = {
    {"verify_rs32", verify_rs32},
    {"verify_rs104", verify_rs104},
    {"resilver_rs32", resilver_rs32},
    {"resilver_rs104", resilver_rs104},
    {"too_few", too_few},
    {"mixed_batch", mixed_batch},
    {"mixed_shapes", mixed_shapes},
    {"shared_location", shared_location},
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
