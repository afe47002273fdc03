// ragged_words_test.cpp — the ragged tier's word layouts and pure host functions
// (csrc/ragged_words.hpp) on the CPU, over seeded random batches, against the properties
// ragged.cpp relies on, written here from their statement: every layout's regions ascending,
// disjoint, aligned to their element and ending at `bytes`; a fill of every region through the
// views staying inside heap buffers of exactly `bytes` (the sanitizer build is the judge); the
// size of a caller-owned words buffer; part_records against a plain loop; sha_list's order.
// Host code only, its own main: built plain by the library's Makefile and with
// -fsanitize=address,undefined by tests/test_ragged_words.py.
#include <cstdio>
#include <memory>
#include <random>

#include "percall_plan.hpp"
#include "ragged_words.hpp"

using namespace cec;

namespace {

int g_failed = 0;

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                               \
        }                                                             \
    } while (0)

// A layout's regions in the order they are meant to lie, checked as they are added and filled
// through a view over two heap buffers of exactly `bytes`.
struct Block {
    explicit Block(size_t bytes)
        : bytes(bytes), h(new uint8_t[bytes]), d(new uint8_t[bytes]), v{h.get(), d.get()} {}
    template <typename T>
    void add(const plan::Region<T>& r) {
        EXPECT(r.off >= end);  // ascending and disjoint
        EXPECT(r.off % sizeof(T) == 0);
        EXPECT(r.end() == r.off + r.count * sizeof(T) && r.end() <= bytes);
        end = r.end();
        T *hp = v.host(r), *dp = v.dev(r);
        for (size_t i = 0; i < r.count; ++i) hp[i] = dp[i] = T(i);
    }
    void add(const plan::ShaListWords& w) {
        EXPECT(end == 0);  // the list opens its buffer: the upload starts at the base
        add(w.ptrs);
        add(w.lens);
        add(w.order);
        EXPECT(w.bytes == end);  // where a tail begins
        // no tail: nothing for nothing hashed, else ptrs and lens whole and the listed items
        const size_t items = w.order.count;
        EXPECT(w.up_bytes(0) == 0 && (!items || w.up_bytes(items) == w.bytes));
        for (size_t hashed = 1; hashed <= items; hashed += 1 + items / 3)
            EXPECT(w.up_bytes(hashed) == items * 16 + hashed * 4);
    }
    void done() { EXPECT(end == bytes); }  // bytes is the end of the last region
    size_t bytes, end = 0;
    std::unique_ptr<uint8_t[]> h, d;
    plan::View v;
};

struct Launch {
    size_t count;
};

void layouts(std::mt19937_64& rng, size_t t, size_t n) {
    const size_t items = n * t;
    // the figure the parts pipeline's slots have had
    const size_t cap = plan::ragged_words_bytes(t, n);
    EXPECT(cap == n * t * 20 + (n + 1) * 4 + n * 24);
    for (int variant = 0; variant < 4; ++variant) {
        const bool fused = variant & 1, split = variant & 2;
        const plan::EncodeWords w = plan::encode_words(t, n, fused, split);
        EXPECT(w.bytes <= cap && (w.bytes == cap) == (!fused && split));
        Block b(w.bytes);
        if (fused) {  // the part order where the SHA-256 list would be
            EXPECT(w.list.order.off == 0 && w.list.order.count == n);
            EXPECT(w.list.ptrs.count == 0 && w.list.lens.count == 0 && w.units.count == 0);
            b.add(w.list.order);
        } else {
            EXPECT(w.list.ptrs.count == items && w.list.lens.count == items);
            EXPECT(w.list.order.count == items && w.units.count == n + 1);
            b.add(w.list);
            b.add(w.units);
        }
        EXPECT(w.parts.count == n * (split ? 6 : 4));
        b.add(w.parts);
        b.done();
    }
    {
        const plan::VerifyWords w = plan::verify_words(items);
        EXPECT(w.list.order.count == items && w.ok.count == items);
        Block b(w.bytes);
        b.add(w.list);
        b.add(w.ok);
        b.done();
    }
    {
        const plan::ReadUpWords w = plan::read_up_words(t, n);
        EXPECT(w.list.order.count == items && w.units.count == n + 1 && w.parts.count == 4 * n);
        EXPECT(w.part_pat.count == n && w.present.count == items);
        Block b(w.bytes);
        b.add(w.list);
        b.add(w.units);
        b.add(w.parts);
        b.add(w.part_pat);
        b.add(w.present);
        b.done();
    }
    for (const bool packed : {false, true}) {
        const size_t slot = 1 + rng() % 80;
        const plan::ReadDevWords w = plan::read_dev_words(t, n, slot, packed);
        EXPECT(w.records.count == n * slot && w.status.count == n && w.ok.count == items);
        EXPECT(w.verified.count == items && w.ret_off.count == (packed ? n + 1 : 0));
        Block b(w.bytes);
        b.add(w.records);
        b.add(w.status);
        b.add(w.ok);
        b.add(w.verified);
        if (packed) {
            EXPECT(w.ret_off.off % 8 == 0 && w.ret_off.off - w.verified.end() < 8);
            b.add(w.ret_off);
        }
        b.done();
    }
    {
        std::vector<Launch> launches;
        for (size_t left = n; left;) {
            launches.push_back({1 + rng() % left});
            left -= launches.back().count;
        }
        const size_t plan_words = rng() % 500;
        const plan::ReconWords w = plan::recon_words(plan_words, launches);
        EXPECT(w.plan.off == 0 && w.plan.count == plan_words);
        EXPECT(w.units.size() == launches.size() && w.parts.size() == launches.size());
        EXPECT(w.bytes == (plan_words + n * 5 + launches.size()) * 4);
        Block b(w.bytes);
        b.add(w.plan);
        for (size_t i = 0; i < launches.size(); ++i) {
            EXPECT(w.units[i].count == launches[i].count + 1);
            EXPECT(w.parts[i].count == 4 * launches[i].count);
            b.add(w.units[i]);
            b.add(w.parts[i]);
        }
        b.done();
    }
}

void records(std::mt19937_64& rng, const std::vector<size_t>& lens, bool with_ids, bool with_disp) {
    const size_t n = lens.size();
    const uint64_t unit = uint64_t(4096) << (rng() % 5);
    std::vector<size_t> offs(n);
    std::vector<uint64_t> disp(n);
    for (size_t k = 0; k < n; ++k) {
        offs[k] = (rng() >> (rng() % 40)) & ~size_t(15);  // both halves in use
        disp[k] = rng();
    }
    std::vector<uint32_t> ids;
    for (size_t k = 0; with_ids && k < n; ++k)
        if (rng() % 3 == 0) ids.push_back(uint32_t(k));
    const size_t count = with_ids ? ids.size() : n, w = with_disp ? 6 : 4;
    std::unique_ptr<uint32_t[]> units(new uint32_t[count + 1]), parts(new uint32_t[w * count]);
    const uint32_t total =
        plan::part_records(unit, offs.data(), lens.data(), with_ids ? ids.data() : nullptr, count,
                           units.get(), parts.get(), with_disp ? disp.data() : nullptr);
    uint64_t acc = 0;
    for (size_t q = 0; q < count; ++q) {
        const size_t k = with_ids ? ids[q] : q;
        const uint32_t* r = parts.get() + w * q;
        EXPECT(units[q] == acc);
        acc += lens[k] / unit + (lens[k] % unit ? 1 : 0);
        EXPECT((uint64_t(r[1]) << 32 | r[0]) == offs[k]);
        EXPECT((uint64_t(r[3]) << 32 | r[2]) == lens[k]);
        if (with_disp) EXPECT((uint64_t(r[5]) << 32 | r[4]) == disp[k]);
    }
    EXPECT(acc <= 0xFFFFFFFFull && units[count] == acc && total == acc);
    // without the prefix array: the same records and total
    std::unique_ptr<uint32_t[]> again(new uint32_t[w * count]);
    EXPECT(plan::part_records(unit, offs.data(), lens.data(), with_ids ? ids.data() : nullptr,
                              count, nullptr, again.get(),
                              with_disp ? disp.data() : nullptr) == total);
    EXPECT(std::equal(again.get(), again.get() + w * count, parts.get()));
}

void sha_lists(std::mt19937_64& rng, const std::vector<size_t>& lens, size_t t, bool pick_all) {
    const size_t n = lens.size(), items = n * t;
    constexpr uint64_t kCanary = 0xC0FFEE0DDBA11ull;
    std::vector<uint8_t> picked(items);
    for (auto& f : picked) f = pick_all || rng() % 3 != 0;
    std::vector<size_t> offs(n);
    for (size_t k = 0; k < n; ++k) offs[k] = size_t(rng() >> 24) & ~size_t(15);
    const uint64_t base = 0x7000000000ull;
    std::unique_ptr<uint64_t[]> ptrs(new uint64_t[items]), h_len(new uint64_t[items]);
    std::unique_ptr<uint32_t[]> order(new uint32_t[items]);
    std::fill(ptrs.get(), ptrs.get() + items, kCanary);
    std::fill(h_len.get(), h_len.get() + items, kCanary);
    std::fill(order.get(), order.get() + items, 0xFFFFFFFFu);
    const size_t count = plan::sha_list(
        lens.data(), n, t, [&](size_t item) { return picked[item] != 0; },
        [&](size_t k, size_t i, size_t cs) { return base + offs[k] + i * cs; }, ptrs.get(),
        h_len.get(), order.get());
    size_t want = 0;
    for (size_t item = 0; item < items; ++item) {
        const size_t k = item / t, i = item % t;
        want += picked[item];
        if (picked[item]) {
            EXPECT(ptrs[item] == base + offs[k] + i * plan::stride16(lens[k]));
            EXPECT(h_len[item] == lens[k]);
        } else {
            EXPECT(ptrs[item] == kCanary && h_len[item] == kCanary);
        }
    }
    EXPECT(count == want);
    std::vector<uint8_t> seen(items);
    for (size_t q = 0; q < items; ++q) {
        if (q >= count) {
            EXPECT(order[q] == 0xFFFFFFFFu);
            continue;
        }
        const uint32_t item = order[q];
        EXPECT(item < items && picked[item] && !seen[item]);  // the picked items, each once
        if (item >= items) continue;
        seen[item] = 1;
        if (!q) continue;
        const uint32_t prev = order[q - 1];
        EXPECT(lens[prev / t] >= lens[item / t]);  // never longer than the one before
        // equal lengths: part order, then chunk order
        if (lens[prev / t] == lens[item / t]) EXPECT(prev < item);
    }
    // the fused kernel's part order: the same rule over the parts
    std::vector<uint32_t> by_len(n);
    plan::length_order(lens.data(), n, by_len.data());
    std::vector<uint8_t> part_seen(n);
    for (size_t q = 0; q < n; ++q) {
        EXPECT(by_len[q] < n && !part_seen[by_len[q]]);
        part_seen[by_len[q]] = 1;
        if (q) EXPECT(lens[by_len[q - 1]] > lens[by_len[q]] ||
                      (lens[by_len[q - 1]] == lens[by_len[q]] && by_len[q - 1] < by_len[q]));
    }
}

// return_guess (percall_plan.hpp) against the rule's statement: in a part with d or more chunks
// loaded, a stride for every slot that is not loaded and that the mode fills.
void guesses(std::mt19937_64& rng, const std::vector<size_t>& lens, size_t t) {
    const size_t n = lens.size(), d = 1 + rng() % t;
    std::vector<uint8_t> present(n * t);
    for (auto& f : present) f = rng() % 4 ? 1 : 0;
    for (const bool data_only : {false, true}) {
        size_t want = 0;
        for (size_t k = 0; k < n; ++k) {
            size_t loaded = 0, fill = 0;
            for (size_t i = 0; i < t; ++i) {
                loaded += present[k * t + i];
                fill += !present[k * t + i] && (i < d || !data_only);
            }
            if (loaded >= d) want += fill * ((lens[k] + 15) / 16 * 16);
        }
        EXPECT(plan::return_guess(d, t, lens.data(), n, present.data(), data_only) == want);
    }
}

}  // namespace

int main() {
    const size_t kLens[] = {1, 15, 16, 17, 4095, 4096, 4097, size_t(1) << 20,
                            (size_t(1) << 32) + 5};
    std::mt19937_64 rng(2718);
    size_t runs = 0;
    for (int rep = 0; rep < 120; ++rep) {
        const size_t t = rep < 2 ? 1 : 1 + rng() % 40;
        const size_t n = rep < 4 ? size_t(rep % 2 ? 300 : 1) : 1 + rng() % 300;
        std::vector<size_t> lens(n);
        for (auto& L : lens) L = kLens[rng() % (sizeof(kLens) / sizeof(kLens[0]))];
        layouts(rng, t, n);
        records(rng, lens, rep & 1, rep & 2);
        sha_lists(rng, lens, t, rep % 3 == 0);
        guesses(rng, lens, t);
        ++runs;
    }
    if (g_failed) {
        std::printf("ragged_words: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ragged_words ok: %zu random batches\n", runs);
    return 0;
}
