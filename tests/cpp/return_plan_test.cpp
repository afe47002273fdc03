// return_plan_test.cpp — the packed return's offset rule (csrc/return_plan.hpp), which
// return_plan_kernel and the host compile alike, on the CPU: ret_bytes and ret_offsets against a
// plain loop written here from the rule's statement (rows * L rounded up to 16 by division, a
// record outside the bound returning nothing), over random records, and the block-wise order the
// kernel sums in (passes of B parts, waves of 64, a carry) against the same offsets.  Host code
// only, its own main: built plain by the library's Makefile and with -fsanitize=address,undefined
// by tests/test_parts_reader_args.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "return_plan.hpp"

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

// The rule as the header of the C-ABI states it.
uint64_t plain_bytes(uint32_t n_out, uint32_t max_rows, uint64_t L) {
    if (n_out > max_rows) return 0;
    const uint64_t stride = (L / 16 + (L % 16 ? 1 : 0)) * 16;
    uint64_t sum = 0;
    for (uint32_t r = 0; r < n_out; ++r) sum += stride;
    return sum;
}

// The kernel's order of summation: passes of `block` parts, an inclusive scan per wave of 64, the
// waves' totals, a carry from pass to pass.
std::vector<uint64_t> blocked_offsets(const std::vector<uint32_t>& n_out,
                                      const std::vector<uint64_t>& L, uint32_t max_rows,
                                      size_t block) {
    const size_t n = n_out.size();
    std::vector<uint64_t> off(n + 1);
    uint64_t carry = 0;
    for (size_t k0 = 0; k0 < n; k0 += block) {
        std::vector<uint64_t> wave_sum(block / 64, 0), inc(block, 0), v(block, 0);
        for (size_t i = 0; i < block; ++i) {
            if (k0 + i < n) v[i] = plan::ret_bytes(n_out[k0 + i], max_rows, L[k0 + i]);
            inc[i] = v[i] + (i % 64 ? inc[i - 1] : 0);
            if (i % 64 == 63) wave_sum[i / 64] = inc[i];
        }
        uint64_t total = 0;
        for (uint64_t s : wave_sum) total += s;
        for (size_t i = 0; i < block && k0 + i < n; ++i) {
            uint64_t before = 0;
            for (size_t w = 0; w < i / 64; ++w) before += wave_sum[w];
            off[k0 + i] = carry + before + inc[i] - v[i];
        }
        carry += total;
    }
    off[n] = carry;
    return off;
}

void run(std::mt19937_64& rng, size_t n, uint32_t max_rows, uint64_t max_len) {
    std::vector<uint32_t> n_out(n);
    std::vector<uint64_t> L(n);
    for (size_t k = 0; k < n; ++k) {
        // mostly within the bound, sometimes past it (a record the planner never writes)
        n_out[k] = uint32_t(rng() % (max_rows + 2)) + (rng() % 50 == 0 ? 1000u : 0u);
        L[k] = 1 + rng() % max_len;
    }
    std::vector<uint64_t> got(n + 1), want(n + 1);
    plan::ret_offsets(n_out.data(), L.data(), n, max_rows, got.data());
    uint64_t acc = 0;
    for (size_t k = 0; k < n; ++k) {
        want[k] = acc;
        acc += plain_bytes(n_out[k], max_rows, L[k]);
        EXPECT(plan::ret_bytes(n_out[k], max_rows, L[k]) == plain_bytes(n_out[k], max_rows, L[k]));
        EXPECT(plan::ret_bytes(n_out[k], max_rows, L[k]) <= uint64_t(max_rows) * plan::ret_stride(L[k]));
    }
    want[n] = acc;
    EXPECT(got == want);
    EXPECT(blocked_offsets(n_out, L, max_rows, 256) == want);
    EXPECT(blocked_offsets(n_out, L, max_rows, 64) == want);
    for (size_t k = 0; k <= n; ++k) EXPECT(got[k] % 16 == 0);
}

}  // namespace

int main() {
    // the stride, at its boundaries
    for (uint64_t L : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull, 65537ull, (1ull << 39) + 1}) {
        EXPECT(plan::ret_stride(L) % 16 == 0);
        EXPECT(plan::ret_stride(L) >= L && plan::ret_stride(L) - L < 16);
    }
    EXPECT(plan::ret_bytes(0, 4, 100) == 0);
    EXPECT(plan::ret_bytes(4, 4, 100) == 4 * 112);
    EXPECT(plan::ret_bytes(5, 4, 100) == 0);  // past the bound: nothing, never more than sized for
    std::mt19937_64 rng(20260);
    size_t runs = 0;
    for (size_t n : {size_t(0), size_t(1), size_t(63), size_t(64), size_t(65), size_t(255),
                     size_t(256), size_t(257), size_t(1025), size_t(4096)})
        for (uint32_t max_rows : {1u, 2u, 4u, 8u})
            for (uint64_t max_len : {17ull, 65537ull, 1ull << 40}) {
                run(rng, n, max_rows, max_len);
                ++runs;
            }
    if (g_failed) {
        std::printf("return_plan: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("return_plan ok: %zu random batches\n", runs);
    return 0;
}
