// plan_math.hpp — the scalar pieces of the on-device decode planner (plan_kernels.hip), written
// so that the host compiles them too: GF(2^8) multiply and inverse without tables, the five
// v_perm table words of a coefficient (pack_coef's, gf256.cpp), and the choice of a part's input
// and output chunks from its verified mask (decode_record's, capi_internal.hpp).
// tests/cpp/plan_math_test.cpp runs them on the CPU against gf256.cpp for every pattern of
// RS(3,2) and RS(5,5).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CEC_HD __host__ __device__ inline
#else
#define CEC_HD inline
#endif

namespace cec {
namespace plan {

// The planner's scope: a lane owns one column of the augmented matrix [A | I] (2d <= 64) and the
// rows of a part fit the shared reconstruct launch (max_var_rows()).
constexpr uint32_t kMaxD = 32;
constexpr uint32_t kMaxP = 8;

// x * 2 in GF(2^8), polynomial 0x11D.
CEC_HD uint32_t gf_xtime(uint32_t a) { return ((a << 1) ^ ((a & 0x80u) ? 0x11Du : 0u)) & 0xFFu; }

// a * b: eight shift-and-add steps, no table (a lone wave waits longer for a dependent table
// load than it spends on these).
CEC_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t acc = 0;
    for (int i = 0; i < 8; ++i) {
        acc ^= (b & 1u) ? a : 0u;
        a = gf_xtime(a);
        b >>= 1;
    }
    return acc;
}

// 1 / a = a^254 (a != 0; 0 for 0).
CEC_HD uint32_t gf_inv(uint32_t a) {
    uint32_t r = 1, sq = a;  // sq = a^(2^i)
    for (int i = 1; i < 8; ++i) {
        sq = gf_mul(sq, sq);
        r = gf_mul(r, sq);
    }
    return r;
}

// pack_coef: {T0.lo, T0.hi, T1.lo, T1.hi, T2} of the coefficient c.  c * e is GF(2)-linear in e,
// so every table entry is an XOR of c * 2^i.
CEC_HD void coef_words(uint32_t c, uint32_t out[5]) {
    uint32_t m[8];  // c * 2^i
    m[0] = c & 0xFFu;
    for (int i = 1; i < 8; ++i) m[i] = gf_xtime(m[i - 1]);
    // entries 0..3 of a table over the bits (a, b): 0, a, b, a ^ b
    auto quad = [](uint32_t a, uint32_t b) { return (a << 8) | (b << 16) | ((a ^ b) << 24); };
    auto splat = [](uint32_t x) { return x * 0x01010101u; };
    out[0] = quad(m[0], m[1]);
    out[1] = quad(m[0], m[1]) ^ splat(m[2]);
    out[2] = quad(m[3], m[4]);
    out[3] = quad(m[3], m[4]) ^ splat(m[5]);
    out[4] = quad(m[6], m[7]);
}

// A part's choice of chunks from `verified` (bit i = chunk i verified), t = d + p chunks:
// in = the first d verified chunks, ascending; out = the unverified data chunks ascending, then
// (unless data_only) the unverified parity chunks ascending, which is the unverified chunks of
// the mode in ascending order.  n_out = 0 for a part that cannot be decoded (fewer than d
// verified) as for one with nothing to rebuild.
struct Choice {
    uint64_t in;     // d bits set (decodable) or fewer
    uint64_t out;
    uint32_t n_out;  // popcount(out), 0 when not decodable
    bool decodable;
};

CEC_HD uint32_t popc64(uint64_t x) { return uint32_t(__builtin_popcountll(x)); }
CEC_HD uint32_t ctz64(uint64_t x) { return uint32_t(__builtin_ctzll(x)); }  // x != 0

CEC_HD Choice choose(uint64_t verified, uint32_t d, uint32_t t, bool data_only) {
    const uint64_t all = t >= 64 ? ~uint64_t(0) : (uint64_t(1) << t) - 1;
    const uint64_t data = (uint64_t(1) << d) - 1;  // d <= 32
    verified &= all;
    Choice c{};
    c.decodable = popc64(verified) >= d;
    uint64_t in = verified;
    for (uint32_t extra = popc64(in); extra > d; --extra)  // drop the highest: at most p steps
        in &= ~(uint64_t(1) << (63 - uint32_t(__builtin_clzll(in))));
    c.in = in;
    c.out = c.decodable ? (~verified & (data_only ? data : all)) : 0;
    c.n_out = popc64(c.out);
    return c;
}

// The index of the r-th set bit of x (r < popcount(x)): at most r + 1 steps.
CEC_HD uint32_t nth_bit(uint64_t x, uint32_t r) {
    for (uint32_t i = 0; i < r; ++i) x &= x - 1;
    return ctz64(x);
}

}  // namespace plan
}  // namespace cec
