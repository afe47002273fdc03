// percall_plan_test.cpp — the per-call tier's layout rules (csrc/percall_plan.hpp) on the CPU:
// the layout of a cec_part_encode batch (one chunk length: the strided block; two or more: the
// split layout) and the byte ranges a host-staged read moves, over seeded random batches, against
// the properties the callers rely on, written here from their statement: every region 16-byte
// aligned and inside the totals the plan reports, the regions pairwise disjoint, staging reserved
// only for unpinned requests, digest offsets slot * (d+p) * 32, and the read's spans ascending,
// disjoint and exactly the loaded / rebuilt chunks.  Host code only, its own main: built plain by
// the library's Makefile and with -fsanitize=address,undefined by tests/test_percall_plan.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "percall_plan.hpp"

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

struct Range {
    size_t lo, hi;
};

// Sorted by start, no two overlap, all inside [0, total).
void expect_disjoint_inside(std::vector<Range> r, size_t total) {
    std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
    for (size_t i = 0; i < r.size(); ++i) {
        EXPECT(r[i].lo % 16 == 0);
        EXPECT(r[i].lo < r[i].hi && r[i].hi <= total);
        if (i) EXPECT(r[i - 1].hi <= r[i].lo);
    }
}

size_t up16(size_t L) { return (L / 16 + (L % 16 ? 1 : 0)) * 16; }
size_t up256(size_t L) { return (L / 256 + (L % 256 ? 1 : 0)) * 256; }

void part_batch(std::mt19937_64& rng, size_t d, size_t p, size_t B, int mode) {
    const size_t t = d + p;
    std::vector<plan::PartIn> in(B);
    const size_t L0 = 1 + rng() % 70000;
    bool distinct = false;
    const bool no_pins = mode == 3 || rng() % 3 == 0;  // a batch that moves in one copy each way
    for (size_t k = 0; k < B; ++k) {
        // mode 0: one length; 1: any lengths; 2: one length but for one request
        size_t L = mode == 1 ? 1 + rng() % 70000 : L0;
        if (mode == 2 && k == B / 2) L = L0 % 70000 + 1;
        const bool pin = !no_pins && rng() % 4 == 0;
        in[k] = {L, pin && rng() % 2, pin && rng() % 2};
        distinct = distinct || L != in[0].L;
    }
    std::vector<plan::PartPlace> at(B);
    plan::PartTotals tot{};
    plan::part_layout(d, p, in.data(), B, at.data(), &tot);
    EXPECT(tot.mixed == distinct);
    EXPECT(tot.dig_bytes == B * t * 32);
    std::vector<Range> dev{{0, tot.dig_bytes}}, sin, sout;
    size_t want_in = 0, want_out = 0;
    bool any_pinned = false;
    for (size_t k = 0; k < B; ++k) {
        const size_t L = in[k].L, cs = distinct ? up16(L) : up256(L);
        EXPECT(at[k].stride == cs);
        EXPECT(at[k].dig_off == k * t * 32);
        dev.push_back({at[k].dev_data, at[k].dev_data + d * cs});
        dev.push_back({at[k].dev_parity, at[k].dev_parity + p * cs});
        if (!in[k].in_pinned) {
            sin.push_back({at[k].in_off, at[k].in_off + d * cs});
            want_in += d * cs;
        }
        if (!in[k].out_pinned) {
            sout.push_back({at[k].out_off, at[k].out_off + p * cs});
            want_out += p * cs;
        }
        any_pinned = any_pinned || in[k].in_pinned || in[k].out_pinned;
        if (!distinct) {  // the [part][d+p][cs] block
            EXPECT(at[k].dev_data == tot.dev_data + k * t * cs);
            EXPECT(at[k].dev_parity == at[k].dev_data + d * cs);
        } else {  // a region each
            EXPECT(at[k].dev_data >= tot.dev_data && at[k].dev_data + d * cs <= tot.dev_parity);
            EXPECT(at[k].dev_parity >= tot.dev_parity);
        }
    }
    expect_disjoint_inside(dev, tot.dev_bytes);
    expect_disjoint_inside(sin, tot.in_bytes);
    // the digest block lies behind the parity in the output staging
    sout.push_back({tot.out_bytes, tot.out_bytes + tot.dig_bytes});
    expect_disjoint_inside(sout, tot.out_bytes + tot.dig_bytes);
    // staging only for what is staged, and no gaps in it
    EXPECT(tot.in_bytes == want_in && tot.out_bytes == want_out);
    EXPECT(tot.dev_data % 256 == 0 && (!distinct || tot.dev_parity % 256 == 0));
    if (distinct && !any_pinned)  // each region moves in one copy: the staging mirrors it
        for (size_t k = 0; k < B; ++k) {
            EXPECT(at[k].in_off == at[k].dev_data - tot.dev_data);
            EXPECT(at[k].out_off == at[k].dev_parity - tot.dev_parity);
        }
}

void read_batch(std::mt19937_64& rng, size_t d, size_t p, size_t n) {
    const size_t t = d + p;
    std::vector<size_t> lens(n), offs(n);
    for (size_t k = 0; k < n; ++k) lens[k] = 1 + rng() % 70000;
    size_t total = 0;
    EXPECT(plan::packed_layout(t, lens.data(), n, offs.data(), &total) == 0);
    std::vector<uint8_t> present(n * t), verified(n * t);
    std::vector<int> status(n);
    for (size_t k = 0; k < n; ++k) {
        size_t good = 0;
        for (size_t i = 0; i < t; ++i) {
            const unsigned r = unsigned(rng() % 8);
            present[k * t + i] = r == 0 ? 0 : r == 1 ? 0x80 : 1;
            verified[k * t + i] = present[k * t + i] && rng() % 8 != 0;
            good += verified[k * t + i];
        }
        status[k] = good >= d ? 0 : 10;
    }
    for (const bool data_only : {true, false}) {
        Spans up, down;
        const size_t up_bytes = plan::loaded_spans(t, lens.data(), offs.data(), n, present.data(), &up);
        const size_t down_bytes = plan::rebuilt_spans(d, t, lens.data(), offs.data(), n,
                                                      verified.data(), status.data(), data_only, &down);
        // the chunks by the rule's statement, in layout order
        Spans want_up, want_down;
        size_t wu = 0, wd = 0;
        for (size_t k = 0; k < n; ++k)
            for (size_t i = 0; i < t; ++i) {
                const size_t at = offs[k] + i * up16(lens[k]);
                if (present[k * t + i]) {
                    want_up.emplace_back(at, at + lens[k]);
                    wu += lens[k];
                }
                if (status[k] == 0 && !verified[k * t + i] && (i < d || !data_only)) {
                    want_down.emplace_back(at, at + lens[k]);
                    wd += lens[k];
                }
            }
        EXPECT(up == want_up && up_bytes == wu);
        EXPECT(down == want_down && down_bytes == wd);
        for (const Spans* s : {&up, &down})
            for (size_t q = 0; q < s->size(); ++q) {
                EXPECT((*s)[q].first < (*s)[q].second && (*s)[q].second <= total);
                if (q) EXPECT((*s)[q - 1].second <= (*s)[q].first);  // ascending, disjoint
            }
    }
    // the layout itself: parts back to back, 16-byte aligned
    size_t end = 0;
    for (size_t k = 0; k < n; ++k) {
        EXPECT(offs[k] == end && offs[k] % 16 == 0);
        end += t * up16(lens[k]);
    }
    EXPECT(total == end);
}

}  // namespace

int main() {
    EXPECT(plan::stride16(1) == 16 && plan::stride16(16) == 16 && plan::stride16(17) == 32);
    EXPECT(plan::stride16(SIZE_MAX) == 0);
    {
        size_t lens[2] = {5, 0}, offs[2], total = 0;
        EXPECT(plan::packed_layout(3, lens, 2, offs, &total) == 1);
        lens[1] = SIZE_MAX / 2;
        EXPECT(plan::packed_layout(3, lens, 2, offs, &total) == 2);
    }
    std::mt19937_64 rng(4608);
    const size_t shapes[4][2] = {{3, 2}, {10, 4}, {20, 8}, {3, 9}};
    size_t runs = 0;
    for (const auto& s : shapes)
        for (int rep = 0; rep < 40; ++rep) {
            const size_t B = rep < 4 ? size_t(rep + 1) : 1 + rng() % 300;
            part_batch(rng, s[0], s[1], B, rep % 4);
            read_batch(rng, s[0], s[1], B);
            ++runs;
        }
    if (g_failed) {
        std::printf("percall_plan: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("percall_plan ok: %zu random batches\n", runs);
    return 0;
}
