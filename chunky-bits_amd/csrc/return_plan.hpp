// return_plan.hpp — the per-part rule of a ragged read's packed return (plan_kernels.hip
// return_plan_kernel, gather_rebuilt_kernel), written so that the host compiles it too: the bytes
// a part's decode record returns.  The region is the parts' returns back to back in part order,
// so the offsets are the exclusive prefix sum of this rule; tests/cpp/return_plan_test.cpp runs it
// and the prefix sum on the CPU against a plain loop over random records.
#pragma once

#include <cstddef>
#include <cstdint>

#include "plan_math.hpp"

namespace cec {
namespace plan {

// L rounded up to 16 (ragged_stride, for lengths that do not overflow it: L <= 2^64 - 16).
CEC_HD uint64_t ret_stride(uint64_t L) { return (L + 15) & ~uint64_t(15); }

// Bytes the record of a part of chunk length L returns: n_out rows (record word 0; 0 = nothing
// rebuilt, or not decodable) of one stride each.  A row count past max_rows (what the host sized
// the region for; decode_plan_kernel never writes one) returns nothing, and the gather skips such
// a part by the same test, so no store can pass the host's bound.
CEC_HD uint64_t ret_bytes(uint32_t n_out, uint32_t max_rows, uint64_t L) {
    return n_out <= max_rows ? uint64_t(n_out) * ret_stride(L) : 0;
}

// ret_off[0 .. n] = the exclusive prefix sum of ret_bytes over n parts (the plain host form of
// return_plan_kernel): n_out[k] = record word 0 of part k, L[k] its chunk length.
inline void ret_offsets(const uint32_t* n_out, const uint64_t* L, size_t n, uint32_t max_rows,
                        uint64_t* ret_off) {
    uint64_t acc = 0;
    for (size_t k = 0; k < n; ++k) {
        ret_off[k] = acc;
        acc += ret_bytes(n_out[k], max_rows, L[k]);
    }
    ret_off[n] = acc;
}

}  // namespace plan
}  // namespace cec
