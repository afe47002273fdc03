// sha256_resume_kernels.hip — resumable SHA-256 of a list of chunk segments on gfx950, for the
// segmented ragged write (cec_encode_hash_segments).  SHA-256 is serial within a chunk, but the
// state after any whole number of 64-byte blocks (the midstate) is all a later launch needs to go
// on: a long chunk passes through as segments, one per launch, and a launch's chain is as long as
// its longest segment, not its longest chunk.
//
//  sha256_resume_kernel  one lane = one segment, one wave per SIMD: sha256_lane_kernel's block
//                        loop (paired 128-byte loads, the next pair in flight while the second
//                        block compresses) between a start that is the initial hash value or the
//                        item's midstate record and an end that is the record again or the
//                        padding and the digest.  List mode only; every launch size takes this
//                        form (there is no producer/rounds split of it).
//  sha256_resume_verify_kernel  the same lane (one template, resume_kernel) for the segmented scrub
//                        (cec_verify_segments): where a chain ends, the eight state words are
//                        compared with the item's expected digest and one flag byte is written;
//                        no digest is stored.
#include "device_common.hpp"
#include "kernels.hpp"
#include "segment_words.hpp"
#include "sha256_device.hpp"

namespace cec {
namespace {

using namespace sha;
using plan::kMidstateBytes;
using plan::kSegFirst;
using plan::kSegLast;

constexpr int kResumeThreads = 256;  // four waves, one per SIMD of a CU (sha256_lane_kernel)

// The end of a chain, by the launch's params: the digest stored (sha256_resume_kernel) ...
__device__ __forceinline__ void finish_chain(const ShaResumeParams& a, uint32_t item,
                                             const uint32_t st[8]) {
    store_digest(a.digests + uint64_t(item) * 32u, st);
}
// ... or compared with the item's expected row, in finish_item's byte order (sha256_kernels.hip),
// and one byte written (sha256_resume_verify_kernel).
__device__ __forceinline__ void finish_chain(const ShaVerifyResumeParams& a, uint32_t item,
                                             const uint32_t st[8]) {
    const uint4* e = reinterpret_cast<const uint4*>(a.expected + uint64_t(item) * 32u);
    const uint4 e0 = e[0], e1 = e[1];
    const bool eq = e0.x == bswap32(st[0]) && e0.y == bswap32(st[1]) && e0.z == bswap32(st[2]) &&
                    e0.w == bswap32(st[3]) && e1.x == bswap32(st[4]) && e1.y == bswap32(st[5]) &&
                    e1.z == bswap32(st[6]) && e1.w == bswap32(st[7]);
    a.ok[item] = eq ? 1 : 0;
}

// One lane's segment, start to end: both kernels are this template, the ending chosen by the
// params' type (finish_chain).  The body stands in the kernel itself: as an inlined function the
// compiler gave the existing kernel another SGPR count (86 for 88).
template <class Params>
__global__ __launch_bounds__(kResumeThreads) void resume_kernel(Params a) {
    extern __shared__ uint32_t cu_reservation[];  // never touched: occupancy control only
    const uint32_t g = blockIdx.x * uint32_t(kResumeThreads) + threadIdx.x;
    if (g >= a.n_items) return;
    const uint32_t item = a.order[g];
    const uint8_t* p = reinterpret_cast<const uint8_t*>(a.ptrs[item]);
    const uint64_t len = a.lens[item];
    const uint32_t fl = a.flags[item];
    // the item's record: only formed into an address here, read unless FIRST, written unless LAST
    uint4* rec = reinterpret_cast<uint4*>(a.midstates + uint64_t(a.record[item]) * kMidstateBytes);
    uint32_t st[8];
    uint64_t prior = 0;
    if (fl & kSegFirst) {
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = kH0[i];
    } else {
        const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        st[0] = r0.x, st[1] = r0.y, st[2] = r0.z, st[3] = r0.w;
        st[4] = r1.x, st[5] = r1.y, st[6] = r1.z, st[7] = r1.w;
        prior = uint64_t(r2.x) | (uint64_t(r2.y) << 32);
    }
    const uint64_t nfull = len >> 6;
    uint32_t w[16];
    if (nfull) {
        // blocks in pairs, both halves of a 128-byte line together (sha256_lane_kernel)
        uint4 q[8];
        load_block<true>(p, q);
        if (nfull > 1) load_block<true>(p + 64, q + 4);
        uint64_t b = 0;
#pragma unroll 1
        for (; b + 1 < nfull; b += 2) {
            block_words(q, w);
            compress(st, w);
            block_words(q + 4, w);
            if (b + 2 < nfull) load_block<true>(p + 64 * (b + 2), q);
            if (b + 3 < nfull) load_block<true>(p + 64 * (b + 3), q + 4);
            compress(st, w);
        }
        if (b < nfull) {  // odd block count: the last full block is in q[0..3]
            block_words(q, w);
            compress(st, w);
        }
    }
    const uint64_t total = prior + len;
    if (!(fl & kSegLast)) {  // len is a multiple of 64 (the host's check): nothing is left over
        rec[0] = make_uint4(st[0], st[1], st[2], st[3]);
        rec[1] = make_uint4(st[4], st[5], st[6], st[7]);
        rec[2] = make_uint4(uint32_t(total), uint32_t(total >> 32), 0u, 0u);
        return;
    }
    const uint32_t rem = uint32_t(len - 64 * nfull);
    const uint32_t tb = tail_blocks(rem);
#pragma unroll 1
    for (uint32_t blk = 0; blk < tb; ++blk) {
        tail_words(p + 64 * nfull, rem, blk, tb, total * 8, w);
        compress(st, w);
    }
    finish_chain(a, item, st);
}

constexpr auto sha256_resume_kernel = &resume_kernel<ShaResumeParams>;
constexpr auto sha256_resume_verify_kernel = &resume_kernel<ShaVerifyResumeParams>;

}  // namespace

namespace {

// One workgroup per 256 items under the lane kernel's reservation rule, whatever the size.
template <class Params>
hipError_t launch_resume(void (*kernel)(Params), bool attr_ok, const Params& a, hipStream_t s) {
    if (a.n_items == 0) return hipSuccess;
    if (!attr_ok) return hipErrorInvalidValue;
    dim3 grid((a.n_items + uint32_t(kResumeThreads) - 1) / uint32_t(kResumeThreads));
    clear_stale_error();
    hipLaunchKernelGGL(kernel, grid, dim3(kResumeThreads), sha_lane_reservation(grid.x), s, a);
    return hipGetLastError();
}

template <class Params>
bool reserve_max(void (*kernel)(Params)) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(sha_lane_reservation_max())) == hipSuccess;
}

}  // namespace

hipError_t launch_sha256_resume(const ShaResumeParams& a, hipStream_t s) {
    if (a.n_items == 0) return hipSuccess;
    static const bool attr_ok = reserve_max(sha256_resume_kernel);
    return launch_resume(sha256_resume_kernel, attr_ok, a, s);
}

hipError_t launch_sha256_resume_verify(const ShaVerifyResumeParams& a, hipStream_t s) {
    if (a.n_items == 0) return hipSuccess;
    static const bool attr_ok = reserve_max(sha256_resume_verify_kernel);
    return launch_resume(sha256_resume_verify_kernel, attr_ok, a, s);
}

}  // namespace cec
