// sha256_kernels.hip — FIPS 180-4 SHA-256 of many chunks on gfx950 (Sha256Hash::from_buf,
// reference src/file/hash/sha256.rs:20-26, called per chunk at src/file/file_part.rs:185 and
// through DataVerifier::verify_async at file_part.rs:102,239,280).
//
// A chunk is a serial chain of 64-byte compressions, so the parallelism is the number of chunks
// (C2: 4096 parts x 14 = 57 344 streams, i.e. under one wave per SIMD).  Measured on MI355X, a
// lone wave issues a VALU op every ~5 cycles at best and a dependent op every ~10-11, and the
// rotate (v_alignbit_b32) and 3-input add (v_add3_u32) that SHA-256 lives on are half-rate ops:
// one wave per SIMD is issue-bound.  Two kernels:
//
//  sha256_lane_kernel   (v1, default) one lane = one chunk, one wave per SIMD.  Message
//                       load, byte swap, message schedule and the 64 rounds all in one wave;
//                       T1 = (h + K[t]+W[t] + Ch) + Sigma1 adds the long-latency Sigma1 last, and
//                       Ch/Maj are single full-rate v_bitop3 (1482 VALU per block, ~4.2 cycles
//                       per instruction per wave measured: near the lone-wave issue floor).
//  sha256_split_kernel  (v2) one 128-thread workgroup = 64 chunks and TWO waves:
//                       wave 0 (producer) loads the block, byte-swaps, expands the message
//                       schedule and writes K[t]+W[t] for block b into an LDS ring slot;
//                       wave 1 (rounds) runs the 64 rounds of block b-1 from the other slot.
//                       One __syncthreads per block hands the slot over.  Doubles the waves
//                       per SIMD, but the half-rate rotate/add3 ops then saturate the shared
//                       SIMDs and the lock-step barrier costs more than it saves (measured
//                       slower than v1; kept as the reference for the producer/consumer split).
#include <cstdlib>

#include "device_common.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "sha256_device.hpp"

namespace cec {
namespace {

using namespace sha;

// Chunk `item` of the launch: pointer and length (strided or list mode).
__device__ __forceinline__ void item_source(const ShaParams& a, uint32_t item, const uint8_t*& p,
                                            uint64_t& len) {
    if (a.ptrs) {
        p = reinterpret_cast<const uint8_t*>(a.ptrs[item]);
        len = a.lens[item];
    } else {
        const uint32_t k = item / a.n_chunks;
        const uint32_t c = item - k * a.n_chunks;
        p = a.base + uint64_t(k) * a.part_stride + uint64_t(a.first_chunk + c) * a.chunk_stride;
        len = a.len;
    }
}

// Digest out and/or compare with the expected digest (verify mode).
__device__ __forceinline__ void finish_item(const ShaParams& a, uint32_t item,
                                            const uint32_t st[8]) {
    if (a.digests) store_digest(a.digests + uint64_t(item) * 32u, st);
    if (a.expected && a.ok) {
        const uint4* e = reinterpret_cast<const uint4*>(a.expected + uint64_t(item) * 32u);
        const uint4 e0 = e[0], e1 = e[1];
        const bool eq = e0.x == bswap32(st[0]) && e0.y == bswap32(st[1]) &&
                        e0.z == bswap32(st[2]) && e0.w == bswap32(st[3]) &&
                        e1.x == bswap32(st[4]) && e1.y == bswap32(st[5]) &&
                        e1.z == bswap32(st[6]) && e1.w == bswap32(st[7]);
        a.ok[item] = eq ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------
// v1: one lane per chunk, everything in one wave
// ------------------------------------------------------------------------------------------

// 256-thread workgroups: the four waves of a workgroup land on the four SIMDs of a CU, and
// launch_sha256 reserves enough (otherwise unused) LDS that at most one such workgroup fits on
// a CU.  The waves of this kernel live for the whole launch, so this pins exactly one wave per
// SIMD whatever ran before: without it, launched behind the encode kernel the dispatcher stacked
// two waves on some SIMDs and the launch took 80 ms instead of 42 ms (C2, MI355X).
constexpr int kLaneThreads = 256;

template <bool VEC>
__global__ __launch_bounds__(kLaneThreads) void sha256_lane_kernel(ShaParams a) {
    extern __shared__ uint32_t cu_reservation[];  // never touched: occupancy control only
    uint32_t item = blockIdx.x * uint32_t(kLaneThreads) + threadIdx.x;
    if (a.items) {
        if (item >= a.n_items) return;
        item = a.items[item];
    } else {
        if (item >= a.n_parts * a.n_chunks) return;
        if (a.present && !a.present[item]) {
            if (a.ok) a.ok[item] = 0;
            return;
        }
    }
    const uint8_t* p;
    uint64_t len;
    item_source(a, item, p, len);
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = kH0[i];
    const uint64_t nfull = len >> 6;
    uint32_t w[16];
    if (nfull) {
        // Blocks are loaded in pairs (one 128-byte line of an aligned chunk), both halves
        // together: every lane streams its own 1 MiB-apart chunk, so the lines of a wave share
        // L2 sets, and a line's second half loaded one block (~2.5 us) later was re-fetched from
        // HBM about half the time (PMC: 1.44-1.72x the algorithmic bytes).  The pair after the
        // current one is in flight while its second block compresses.
        uint4 q[8];
        load_block<VEC>(p, q);
        if (nfull > 1) load_block<VEC>(p + 64, q + 4);
        uint64_t b = 0;
#pragma unroll 1
        for (; b + 1 < nfull; b += 2) {
            block_words(q, w);
            compress(st, w);
            block_words(q + 4, w);
            if (b + 2 < nfull) load_block<VEC>(p + 64 * (b + 2), q);
            if (b + 3 < nfull) load_block<VEC>(p + 64 * (b + 3), q + 4);
            compress(st, w);
        }
        if (b < nfull) {  // odd block count: the last full block is in q[0..3]
            block_words(q, w);
            compress(st, w);
        }
    }
    const uint32_t rem = uint32_t(len - 64 * nfull);
    const uint32_t tb = tail_blocks(rem);
#pragma unroll 1
    for (uint32_t blk = 0; blk < tb; ++blk) {
        tail_words(p + 64 * nfull, rem, blk, tb, len * 8, w);
        compress(st, w);
    }
    finish_item(a, item, st);
}

// ------------------------------------------------------------------------------------------
// v2: producer (schedule) wave + rounds wave per 64 chunks, K+W handed over through LDS
// ------------------------------------------------------------------------------------------

// One lane's K+W row: 64 words + 4 pad words -> 272-byte stride, so the 16 lanes of each
// ds_read_b128 / ds_write_b128 lane group cover all 64 banks exactly once.
constexpr int kKwRow = 68;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, uint32_t(__shfl_xor(int(v), m, 64)));
    return v;
}

// SPW = streams per wave.
template <bool VEC, int SPW>
__global__ __launch_bounds__(128) void sha256_split_kernel(ShaParams a) {
    __shared__ __attribute__((aligned(16))) uint32_t kw[2][SPW * kKwRow];
    const uint32_t lane = threadIdx.x & 63u;
    const bool producer = threadIdx.x < 64u;  // wave-uniform
    const uint32_t idx = blockIdx.x * uint32_t(SPW) + lane;
    bool valid = lane < uint32_t(SPW) &&
                 idx < (a.items ? a.n_items : a.n_parts * a.n_chunks);
    const uint32_t item = valid && a.items ? a.items[idx] : idx;
    bool skipped = false;  // verify mode, chunk not loaded: no blocks, ok = 0
    if (valid && !a.items && a.present && !a.present[item]) {
        skipped = true;
        valid = false;
    }
    const uint8_t* p = nullptr;
    uint64_t len = 0;
    if (valid) item_source(a, item, p, len);
    const uint64_t nfull = len >> 6;
    const uint32_t rem = uint32_t(len - 64 * nfull);
    const uint32_t nb = valid ? uint32_t(nfull) + tail_blocks(rem) : 0u;
    // Both waves hold the same 64 items, so both compute the same trip count: every lane of
    // the workgroup reaches the same number of barriers.
    const uint32_t nb_max = wave_max_u32(nb);

    if (producer) {
        // Blocks loaded in pairs, both halves of a 128-byte line together (see the lane kernel).
        uint4 q[8];
        if (nfull) load_block<VEC>(p, q);
        if (nfull > 1) load_block<VEC>(p + 64, q + 4);
#pragma unroll 1
        for (uint32_t b = 0; b <= nb_max; ++b) {
            if (b < nb) {
                uint32_t w[16];
                if (b < nfull) {
                    if (b & 1) {  // wave-uniform: static register indexing in both arms
                        block_words(q + 4, w);
                        if (b + 1 < nfull) load_block<VEC>(p + 64 * uint64_t(b + 1), q);
                        if (b + 2 < nfull) load_block<VEC>(p + 64 * uint64_t(b + 2), q + 4);
                    } else {
                        block_words(q, w);
                    }
                } else {
                    tail_words(p + 64 * nfull, rem, b - uint32_t(nfull), tail_blocks(rem),
                               len * 8, w);
                }
                uint32_t* row = &kw[b & 1][(lane % SPW) * kKwRow];
#pragma unroll
                for (int i = 0; i < 64; i += 4) {
                    uint32_t v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        v[k] = (i + k < 16 ? w[i + k] : schedule_next(w, i + k)) + kK[i + k];
                    *reinterpret_cast<uint4*>(row + i) = make_uint4(v[0], v[1], v[2], v[3]);
                }
            }
            __syncthreads();
        }
    } else {
        uint32_t st[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = kH0[i];
#pragma unroll 1
        for (uint32_t b = 0; b <= nb_max; ++b) {
            if (b >= 1 && b - 1 < nb) {
                const uint32_t* row = &kw[(b - 1) & 1][(lane % SPW) * kKwRow];
                uint32_t x0 = st[0], x1 = st[1], x2 = st[2], x3 = st[3];
                uint32_t x4 = st[4], x5 = st[5], x6 = st[6], x7 = st[7];
#pragma unroll
                for (int i = 0; i < 64; i += 4) {
                    const uint4 v = *reinterpret_cast<const uint4*>(row + i);
                    round_step(x0, x1, x2, x3, x4, x5, x6, x7, v.x);
                    round_step(x0, x1, x2, x3, x4, x5, x6, x7, v.y);
                    round_step(x0, x1, x2, x3, x4, x5, x6, x7, v.z);
                    round_step(x0, x1, x2, x3, x4, x5, x6, x7, v.w);
                }
                st[0] += x0;
                st[1] += x1;
                st[2] += x2;
                st[3] += x3;
                st[4] += x4;
                st[5] += x5;
                st[6] += x6;
                st[7] += x7;
            }
            __syncthreads();
        }
        if (valid) finish_item(a, item, st);
        else if (skipped && a.ok) a.ok[item] = 0;
    }
}

// CEC_SHA_VARIANT (test knob): 1 = lane kernel, 2 = split kernel (both correct; by size when
// unset).  Any other value counts as unset.
int sha_variant() {
    const int v = knobs().sha_variant;
    return v == 1 || v == 2 ? v : 0;
}

// Dynamic LDS requested per lane-kernel workgroup: more than half of the 160 KiB of a CU, so
// two workgroups never share a CU.
constexpr size_t kCuReservation = 96 * 1024;
// ... and at most two (grids larger than one workgroup per CU).
constexpr size_t kCuReservation2 = 64 * 1024;

hipError_t launch_lane(const ShaParams& a, bool vec16, hipStream_t s) {
    static const bool attr_ok = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&sha256_lane_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   int(kCuReservation)) == hipSuccess &&
               hipFuncSetAttribute(reinterpret_cast<const void*>(&sha256_lane_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   int(kCuReservation)) == hipSuccess;
    }();
    if (!attr_ok) return hipErrorInvalidValue;
    const uint64_t total = a.items ? a.n_items : uint64_t(a.n_parts) * a.n_chunks;
    dim3 grid(uint32_t((total + kLaneThreads - 1) / kLaneThreads));
    // One workgroup (one wave per SIMD) per CU while the grid fits the chip in one pass.  When
    // it does not, a second co-resident wave per SIMD turns the lone wave's issue-bound ~6000
    // cycles per block into a shared SIMD-bound ~5100 per wave: every wave starts at once
    // instead of a second, partly empty pass.
    const size_t lds = grid.x > uint32_t(device_cus()) ? kCuReservation2 : kCuReservation;
    clear_stale_error();
    if (vec16)
        hipLaunchKernelGGL((sha256_lane_kernel<true>), grid, dim3(kLaneThreads), lds, s, a);
    else
        hipLaunchKernelGGL((sha256_lane_kernel<false>), grid, dim3(kLaneThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_split(const ShaParams& a, bool vec16, hipStream_t s) {
    const uint64_t total = a.items ? a.n_items : uint64_t(a.n_parts) * a.n_chunks;
    dim3 grid(uint32_t((total + 63) / 64));
    clear_stale_error();
    if (vec16) hipLaunchKernelGGL((sha256_split_kernel<true, 64>), grid, dim3(128), 0, s, a);
    else hipLaunchKernelGGL((sha256_split_kernel<false, 64>), grid, dim3(128), 0, s, a);
    return hipGetLastError();
}

}  // namespace

// The lane kernel's one-wave-per-SIMD reservation (launch_lane's rule), for the other lane-per-item
// kernels (sha256_resume_kernels.hip): the dynamic LDS a 256-thread workgroup of a grid of
// `grid_x` workgroups asks for, and the most it ever asks for (the kernel's attribute).
size_t sha_lane_reservation(uint32_t grid_x) {
    return grid_x > uint32_t(device_cus()) ? kCuReservation2 : kCuReservation;
}
size_t sha_lane_reservation_max() { return kCuReservation; }

// CUs of the current device (cached per device ordinal); 256 when unknown.
int device_cus() {
    static std::atomic<uint32_t> cache[kMaxDevices];
    return int(per_device(cache, 256u, [](int dev) {
        int n = 0;
        return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) ==
                           hipSuccess && n > 0 ? uint32_t(n) : 256u;
    }));
}

// Chunks up to which a launch takes the split kernel: its 2 waves per 64 chunks then fill at
// most a quarter of the SIMDs (4 x CUs), leaving room for the other launches in flight (write /
// read pipeline slots, coalesced per-call batches: 4 each).  Past it the chip fills and the lane
// kernel's one wave per 64 chunks wins (C2: split 50.6 ms vs lane 42.1 ms).
uint64_t split_max_chunks() { return uint64_t(device_cus()) * 32; }

bool use_split(uint64_t chunks) {
    const int v = sha_variant();
    if (v) return v == 2;
    return chunks <= split_max_chunks();
}

// By size (use_split) unless CEC_SHA_VARIANT forces one: the lane kernel (one lane per chunk) or
// the split producer/rounds waves.  A lone 1 MiB chain: lane kernel ~42 ms, split kernel ~31 ms
// (rounds wave alone on its SIMD; profiles/r1z_sha_ab_small.log).
hipError_t launch_sha256(const ShaParams& a, bool vec16, hipStream_t s) {
    const uint64_t total = a.items ? a.n_items : uint64_t(a.n_parts) * a.n_chunks;
    if (total == 0) return hipSuccess;
    if (use_split(total)) return launch_split(a, vec16, s);
    return launch_lane(a, vec16, s);
}

}  // namespace cec
