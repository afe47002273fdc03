// plan_math_test.cpp — the scalar pieces of the on-device decode planner (csrc/plan_math.hpp) on
// the CPU, against the host's own arithmetic (csrc/gf256.cpp): gf_mul / gf_inv against the
// exp/log tables for every operand, coef_words against pack_coef for every coefficient, and, for
// every verified set of RS(3,2) and RS(5,5) in both modes, the record the planner's steps give
// (choose, a column-wise Gauss-Jordan with gf_mul / gf_inv, coef_words) against write_pattern
// over invert, word for word.  Host code only; tests/test_ragged_read_async.py runs it plain and
// built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gf256.hpp"
#include "plan_math.hpp"

using namespace cec;

namespace {

int g_failures = 0;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (++g_failures <= 20) {         \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

// The record of a verified set as the host builds it (cec_codec::decode_record's rule, restated):
// empty when fewer than d chunks verified or nothing is to be rebuilt.
std::vector<uint32_t> host_record(const ByteMatrix& m, size_t d, size_t p, uint64_t verified,
                                  bool data_only) {
    const size_t t = d + p;
    std::vector<uint32_t> in_idx, out_idx, miss_par;
    size_t good = 0;
    for (size_t i = 0; i < t; ++i) {
        if ((verified >> i) & 1) {
            ++good;
            if (in_idx.size() < d) in_idx.push_back(uint32_t(i));
        } else if (i < d) {
            out_idx.push_back(uint32_t(i));
        } else if (!data_only) {
            miss_par.push_back(uint32_t(i));
        }
    }
    out_idx.insert(out_idx.end(), miss_par.begin(), miss_par.end());
    if (good < d || out_idx.empty()) return {0};
    ByteMatrix sub(d, d), dec;
    for (size_t r = 0; r < d; ++r)
        for (size_t c = 0; c < d; ++c) sub.at(r, c) = m.at(in_idx[r], c);
    if (!invert(sub, dec)) return {0};
    ByteMatrix pick(out_idx.size(), d);
    for (size_t k = 0; k < out_idx.size(); ++k)
        for (size_t c = 0; c < d; ++c) pick.at(k, c) = m.at(out_idx[k], c);
    // M[o] * inv(M[in]) is the inverse's row o for a data chunk (M's top is the identity)
    const ByteMatrix rows = multiply(pick, dec);
    std::vector<uint32_t> rec(pattern_words(d, out_idx.size()));
    write_pattern(rec.data(), d, in_idx, out_idx, rows);
    return rec;
}

// The same record by the planner's steps: lane c's column is w[.][c].
std::vector<uint32_t> planned_record(const ByteMatrix& m, size_t d, size_t p, uint64_t verified,
                                     bool data_only, size_t max_rows) {
    const uint32_t t = uint32_t(d + p);
    const plan::Choice ch = plan::choose(verified, uint32_t(d), t, data_only);
    if (ch.n_out == 0 || ch.n_out > max_rows) return {0};
    std::vector<std::vector<uint8_t>> w(d, std::vector<uint8_t>(2 * d, 0));
    for (size_t r = 0; r < d; ++r) {
        const uint32_t src = plan::nth_bit(ch.in, uint32_t(r));
        for (size_t c = 0; c < d; ++c) w[r][c] = m.at(src, c);
        w[r][d + r] = 1;
    }
    for (size_t c = 0; c < d; ++c) {
        size_t piv = d;
        for (size_t r = d; r-- > c;)
            if (w[r][c]) piv = r;
        if (piv >= d) return {0};
        const uint32_t scale = plan::gf_inv(w[piv][c]);
        std::vector<uint8_t> factor(d);
        for (size_t r = 0; r < d; ++r) factor[r] = w[r == c ? piv : r == piv ? c : r][c];
        for (size_t lane = 0; lane < 2 * d; ++lane) {
            const uint32_t top = w[c][lane], low = w[piv][lane];
            w[piv][lane] = uint8_t(top);
            const uint32_t pc = plan::gf_mul(scale, low);
            w[c][lane] = uint8_t(pc);
            for (size_t r = 0; r < d; ++r)
                if (r != c) w[r][lane] = uint8_t(w[r][lane] ^ plan::gf_mul(factor[r], pc));
        }
    }
    const size_t n_out = ch.n_out;
    std::vector<uint32_t> rec(pattern_words(d, n_out));
    rec[0] = uint32_t(n_out);
    for (size_t j = 0; j < d; ++j) rec[1 + j] = plan::nth_bit(ch.in, uint32_t(j));
    for (size_t r = 0; r < n_out; ++r) rec[1 + d + r] = plan::nth_bit(ch.out, uint32_t(r));
    for (size_t j = 0; j < d; ++j)
        for (size_t r = 0; r < n_out; ++r) {
            const uint32_t o = plan::nth_bit(ch.out, uint32_t(r));
            uint32_t coef = 0;
            if (o < d) {
                coef = w[o][d + j];
            } else {
                for (size_t q = 0; q < d; ++q) coef ^= plan::gf_mul(m.at(o, q), w[q][d + j]);
            }
            plan::coef_words(coef, rec.data() + 1 + d + n_out + (j * n_out + r) * kTabWords);
        }
    return rec;
}

void check_shape(size_t d, size_t p) {
    const ByteMatrix m = build_coding_matrix(d, p);
    const size_t t = d + p;
    size_t decodable = 0, planned = 0;
    for (int data_only = 0; data_only < 2; ++data_only) {
        const size_t max_rows = data_only ? (p < d ? p : d) : p;
        for (uint64_t v = 0; v < (uint64_t(1) << t); ++v) {
            const std::vector<uint32_t> want = host_record(m, d, p, v, data_only != 0);
            const std::vector<uint32_t> got = planned_record(m, d, p, v, data_only != 0, max_rows);
            CHECK(got == want, "RS(%zu,%zu) verified %#llx data_only %d", d, p,
                  (unsigned long long)v, data_only);
            const plan::Choice ch = plan::choose(v, uint32_t(d), uint32_t(t), data_only != 0);
            const bool ok = size_t(__builtin_popcountll(v)) >= d;
            CHECK(ch.decodable == ok, "RS(%zu,%zu) verified %#llx", d, p, (unsigned long long)v);
            CHECK(ch.n_out <= max_rows, "RS(%zu,%zu) verified %#llx: %u rows", d, p,
                  (unsigned long long)v, ch.n_out);
            if (!data_only && ok) ++decodable;
            if (want[0]) ++planned;
        }
    }
    std::printf("RS(%zu,%zu): %zu verified sets with >= d chunks, %zu records compared\n", d, p,
                decodable, planned);
}

}  // namespace

int main() {
    const Gf256& g = Gf256::get();
    for (unsigned a = 0; a < 256; ++a) {
        for (unsigned b = 0; b < 256; ++b)
            CHECK(plan::gf_mul(a, b) == g.mul(uint8_t(a), uint8_t(b)), "mul %u %u", a, b);
        if (a) CHECK(plan::gf_inv(a) == g.div(1, uint8_t(a)), "inv %u", a);
        uint32_t want[kTabWords], got[kTabWords];
        pack_coef(uint8_t(a), want);
        plan::coef_words(a, got);
        for (int x = 0; x < kTabWords; ++x) CHECK(got[x] == want[x], "coef %u word %d", a, x);
    }
    CHECK(plan::gf_inv(0) == 0, "inv 0");
    check_shape(3, 2);
    check_shape(5, 5);
    check_shape(1, 1);
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("plan_math ok\n");
    return 0;
}
