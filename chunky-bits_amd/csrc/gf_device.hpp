// gf_device.hpp — GF(2^8) multiply-by-constant for gfx950 via v_perm_b32 byte tables (layout
// of the 5 packed table words: gf256.hpp pack_coef).  Shared by rs_kernels.hip and the fused
// encode+hash kernel.
#pragma once

#include "device_common.hpp"
#include "gf256.hpp"

namespace cec {
namespace gf {

// Rows [row0, n_out) of the pattern record `pat` (d inputs, n_out rows; layout: gf256.hpp).
// tab is row0's table of input 0; input j's tables for these rows start at tab + j*tab_stride.
struct PatView {
    cu32* in_idx;
    cu32* out_idx;
    cu32* tab;
    uint32_t tab_stride;
    __device__ __forceinline__ PatView(cu32* pat, uint32_t d, uint32_t n_out, uint32_t row0 = 0)
        : in_idx(pat + 1),
          out_idx(pat + 1 + d + row0),
          tab(pat + 1 + d + n_out + size_t(row0) * kTabWords),
          tab_stride(n_out * kTabWords) {}
};

struct Sel {
    uint32_t s0, s1, s2;
};

__device__ __forceinline__ Sel selectors(uint32_t x) {
    return {x & 0x07070707u, (x >> 3) & 0x07070707u, (x >> 6) & 0x03030303u};
}

// c (x) x for 4 packed bytes, c given by its 5 packed table words.
__device__ __forceinline__ uint32_t gmul(const Sel& s, uint32_t t0, uint32_t t1, uint32_t t2,
                                         uint32_t t3, uint32_t t4) {
    return xor3(perm(t1, t0, s.s0), perm(t3, t2, s.s1), perm(0u, t4, s.s2));
}

}  // namespace gf
}  // namespace cec
