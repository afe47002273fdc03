// plan_kernels.hip — the decode plan of a ragged read, built on the device.
//
// cec_read_ragged plans its rebuild on the host, between the verification and the decode: it
// waits for the flags, groups the parts by erasure pattern, inverts a matrix per pattern and
// uploads the records.  Everything in that plan is a function of the flags, which are on the
// device already, and of the codec's coding matrix, so decode_plan_kernel computes it there and
// the whole read is one enqueue (ragged.cpp read_ragged_async).
//
// One WAVE per part.  The wave's verified set is one 64-bit ballot; from it every lane derives
// the same input and output chunks (plan_math.hpp choose, wave-uniform).  The inversion is
// Gauss-Jordan over the augmented matrix [A | I], A = the rows of M of the d input chunks: lane c
// owns column c (2d <= 64 columns) and keeps it in LDS, which it alone reads and writes, so no
// lane ever waits for another's store; the pivot row, the pivot value and each row's factor come
// from the lane that owns the pivot column through a shuffle.  Every loop is bounded by d, the
// pivot search included: a column without a pivot (impossible for rows of M, which are
// independent) ends the part with an empty record, as an undecodable part does.
// The lanes of the right half then hold the columns of the inverse: lane d + j computes, for
// every output row, the coefficient of input j (a row of the inverse for a data chunk, M[o] times
// the inverse for a parity chunk) and stores its five table words where write_pattern puts them.
// GF(2^8) arithmetic is exact and the inverse unique, so the record equals the host's
// (cec_codec::decode_record) word for word whatever the elimination order.
#include <hip/hip_runtime.h>

#include "chunky_ec.h"
#include "device_common.hpp"
#include "gf256.hpp"
#include "kernels.hpp"
#include "plan_math.hpp"
#include "return_plan.hpp"

namespace cec {
namespace {

constexpr uint32_t kPlanThreads = 256;
constexpr uint32_t kPlanWaves = kPlanThreads / 64;

// A 32-bit value of lane `src` (wave-uniform), in every lane.
__device__ __forceinline__ uint32_t from_lane(uint32_t v, uint32_t src) {
    return uint32_t(__shfl(int(v), int(src), 64));
}

__global__ __launch_bounds__(kPlanThreads) void decode_plan_kernel(PlanParams a) {
    // column c of wave w's augmented matrix: col[w][r][c], touched by lane c only
    __shared__ uint8_t col[kPlanWaves][plan::kMaxD][64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t k = __builtin_amdgcn_readfirstlane(blockIdx.x * kPlanWaves + w);
    if (k >= a.n_parts) return;  // wave-uniform
    const uint32_t d = a.d, t = a.d + a.p;

    // verified flags (rebuild_mask's rule) and the part's status
    uint32_t ver = 0;
    if (lane < t) {
        const uint64_t x = uint64_t(k) * t + lane;
        const uint8_t f = a.present[x];
        ver = f == CEC_PRESENT_VERIFIED ? 1u : f != 0 ? (a.ok[x] != 0 ? 1u : 0u) : 0u;
        a.verified[x] = uint8_t(ver);
    }
    const uint64_t mask = __ballot(ver != 0);
    const plan::Choice ch = plan::choose(mask, d, t, a.data_only != 0);
    uint32_t* rec = a.records + uint64_t(k) * a.slot_words;
    if (lane == 0) {
        a.part_status[k] = ch.decodable ? CEC_OK : CEC_TOO_FEW_SHARDS_PRESENT;
        rec[0] = 0;  // until the record is complete: rs_reconstruct_ragged_kernel skips the part
    }
    const uint32_t n_out = ch.n_out;
    if (n_out == 0 || n_out > a.max_rows) return;  // wave-uniform; the second cannot happen

    // [A | I]: A[r] = M[in_idx[r]]
    uint8_t(*my)[64] = col[w];
    {
        uint64_t in = ch.in;
        for (uint32_t r = 0; r < d; ++r) {
            const uint32_t src = plan::ctz64(in);
            in &= in - 1;
            uint8_t v = 0;
            if (lane < d) v = a.matrix[src * d + lane];
            else if (lane < 2 * d) v = lane - d == r ? 1 : 0;
            my[r][lane] = v;
        }
    }
    bool singular = false;
    for (uint32_t c = 0; c < d; ++c) {
        // the first row at or below the diagonal with a nonzero entry in column c: lane c looks
        uint32_t piv = d;
        if (lane == c)
            for (uint32_t r = d; r-- > c;)
                if (my[r][lane]) piv = r;
        piv = from_lane(piv, c);
        if (piv >= d) {
            singular = true;
            break;
        }
        const uint32_t top = my[c][lane], low = my[piv][lane];  // swap rows c and piv
        my[piv][lane] = uint8_t(top);
        const uint32_t scale = plan::gf_inv(from_lane(low, c));
        const uint32_t pc = plan::gf_mul(scale, low);  // the scaled pivot row, this column
        my[c][lane] = uint8_t(pc);
        for (uint32_t r = 0; r < d; ++r) {
            const uint32_t v = my[r][lane];
            const uint32_t f = from_lane(v, c);
            if (r != c) my[r][lane] = uint8_t(v ^ plan::gf_mul(f, pc));
        }
    }
    if (singular) return;  // wave-uniform: the record stays empty

    // the record, in write_pattern's layout
    if (lane < d) rec[1 + lane] = plan::nth_bit(ch.in, lane);
    if (lane < n_out) rec[1 + d + lane] = plan::nth_bit(ch.out, lane);
    if (lane >= d && lane < 2 * d) {
        const uint32_t j = lane - d;  // column j of the inverse is this lane's
        uint32_t* tab = rec + 1 + d + n_out + size_t(j) * n_out * kTabWords;
        uint64_t out = ch.out;
        for (uint32_t r = 0; r < n_out; ++r) {
            const uint32_t o = plan::ctz64(out);
            out &= out - 1;
            uint32_t coef = 0;
            if (o < d) {
                coef = my[o][lane];
            } else {
                for (uint32_t q = 0; q < d; ++q)
                    coef ^= plan::gf_mul(a.matrix[o * d + q], my[q][lane]);
            }
            uint32_t words[kTabWords];
            plan::coef_words(coef, words);
#pragma unroll
            for (int x = 0; x < kTabWords; ++x) tab[r * kTabWords + x] = words[x];
        }
    }
    if (lane == 0) rec[0] = n_out;
}

// ------------------------------------------------------------------------------------------
// The packed return of a ragged read: what the rebuild wrote, gathered into one
// dense region in part order, so the copy back to the host is exactly those bytes.
//
// return_plan_kernel: ONE workgroup walks the parts in passes of kRetThreads, a part per thread:
// the part's return (return_plan.hpp ret_bytes of its record's row count and its chunk length),
// an inclusive scan inside each wave by shuffles, the waves' totals through LDS, and a carry
// from pass to pass that every thread keeps (the same sum in each, so it is uniform).  No other
// workgroup exists, nothing waits for anything but the two barriers of a pass, and the one loop
// is bounded by n_parts.  Offsets are 64-bit bytes.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kRetThreads = 256;
constexpr uint32_t kRetWaves = kRetThreads / 64;

__global__ __launch_bounds__(kRetThreads) void return_plan_kernel(ReturnParams a) {
    __shared__ uint64_t wave_sum[kRetWaves];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t carry = 0;  // bytes of the parts of the passes so far
    for (uint32_t k0 = 0; k0 < a.n_parts; k0 += kRetThreads) {  // block-uniform
        const uint32_t k = k0 + threadIdx.x;
        uint64_t v = 0;
        if (k < a.n_parts) {
            const uint32_t* pm = a.parts + size_t(k) * 4;
            const uint64_t L = uint64_t(pm[2]) | (uint64_t(pm[3]) << 32);
            v = plan::ret_bytes(a.records[uint64_t(k) * a.slot_words], a.max_rows, L);
        }
        uint64_t inc = v;  // inclusive scan over the wave
#pragma unroll
        for (uint32_t step = 1; step < 64; step <<= 1) {
            const uint64_t below = __shfl_up(static_cast<unsigned long long>(inc), step, 64);
            if (lane >= step) inc += below;
        }
        if (lane == 63) wave_sum[w] = inc;
        __syncthreads();
        uint64_t before = 0, total = 0;
#pragma unroll
        for (uint32_t i = 0; i < kRetWaves; ++i) {
            const uint64_t s = wave_sum[i];
            before += i < w ? s : 0;
            total += s;
        }
        if (k < a.n_parts) a.ret_off[k] = carry + before + inc - v;
        carry += total;
        __syncthreads();  // wave_sum is written again by the next pass
    }
    if (threadIdx.x == 0) a.ret_off[a.n_parts] = carry;
}

// gather_rebuilt_kernel: one WAVE per (work unit, output row), the units and the wave's search
// for its part those of the rebuild launch (rs_kernels.hip wave_unit): grid.x covers the layout's
// units, grid.y = max_rows.  A wave whose row is at or past its part's row count (or whose record
// is outside the host's bound, as ret_bytes) exits at once; the others copy their unit's columns
// of chunk rec[1 + d + row] to row `row` of the part's place in the region: 16 bytes per lane and
// step, the chunk's last 1..15 bytes by one lane byte for byte.  Exactly L bytes of a row are
// written, all inside [ret_off[k], ret_off[k + 1]).  Plain loads (the rebuild has just written
// these lines) and plain stores (the copy to the host reads them next).
constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kGatherWaves = kGatherThreads / 64;
constexpr uint64_t kGatherStep = 64u * 16u;  // bytes per wave per step

__global__ __launch_bounds__(kGatherThreads) void gather_rebuilt_kernel(ReturnParams a) {
    const uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * kGatherWaves +
                                                      (threadIdx.x >> 6));
    if (u >= a.total_units) return;  // wave-uniform
    cu32* pre = as_const(a.units);
    uint32_t lo = 0, hi = a.n_parts;  // pre[lo] <= u < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= u) lo = mid;
        else hi = mid;
    }
    const uint32_t k = lo, row = blockIdx.y;
    cu32* rec = as_const(a.records) + uint64_t(k) * a.slot_words;
    const uint32_t n_out = rec[0];
    if (row >= n_out || n_out > a.max_rows) return;  // wave-uniform
    const uint32_t chunk = rec[1 + a.d + row];
    if (chunk >= a.t) return;  // not a record of this codec: nothing is read
    cu32* pm = as_const(a.parts) + size_t(k) * 4;
    const uint64_t off = uint64_t(pm[0]) | (uint64_t(pm[1]) << 32);
    const uint64_t len = uint64_t(pm[2]) | (uint64_t(pm[3]) << 32);
    const uint64_t cs = plan::ret_stride(len);
    cu32* ro = as_const(reinterpret_cast<const uint32_t*>(a.ret_off)) + size_t(k) * 2;
    const uint64_t at = uint64_t(ro[0]) | (uint64_t(ro[1]) << 32);
    const uint8_t* src = a.base + off + chunk * cs;
    uint8_t* dst = a.rebuilt + at + row * cs;
    const uint64_t x0 = uint64_t(u - pre[k]) * a.unit_bytes;
    const uint64_t x1 = x0 + a.unit_bytes < len ? x0 + a.unit_bytes : len;
    const uint64_t lane_x = uint64_t(threadIdx.x & 63u) * 16u;
#pragma unroll 1
    for (uint64_t xb = x0; xb < x1; xb += kGatherStep) {  // wave-uniform
        const uint64_t x = xb + lane_x;
        if (x + 16 <= len) {
            *reinterpret_cast<uint4*>(dst + x) = *reinterpret_cast<const uint4*>(src + x);
        } else if (x < len) {
            for (uint64_t b = x; b < len; ++b) dst[b] = src[b];  // at most 15 bytes
        }
    }
}

}  // namespace

bool decode_plan_covers(uint32_t d, uint32_t p) {
    return d >= 1 && d <= plan::kMaxD && p >= 1 && p <= plan::kMaxP;
}

hipError_t launch_decode_plan(const PlanParams& a, hipStream_t s) {
    if (a.n_parts == 0) return hipSuccess;
    if (!decode_plan_covers(a.d, a.p) || a.max_rows > max_var_rows() ||
        a.slot_words < pattern_words(a.d, a.max_rows) || !a.present || !a.ok || !a.matrix ||
        !a.verified || !a.part_status || !a.records)
        return hipErrorInvalidValue;
    const dim3 grid((a.n_parts + kPlanWaves - 1) / kPlanWaves);
    clear_stale_error();
    hipLaunchKernelGGL(decode_plan_kernel, grid, dim3(kPlanThreads), 0, s, a);
    return hipGetLastError();
}

// Both kernels of the packed return, the scan first.
hipError_t launch_return_plan(const ReturnParams& a, hipStream_t s) {
    if (a.n_parts == 0) return hipSuccess;
    if (!a.base || !a.records || !a.units || !a.parts || !a.ret_off || !a.rebuilt ||
        a.max_rows == 0 || a.max_rows > plan::kMaxP || a.slot_words < 1 + a.d + a.max_rows ||
        a.unit_bytes == 0 || a.unit_bytes % kGatherStep || a.total_units > ragged_max_units() ||
        reinterpret_cast<uintptr_t>(a.rebuilt) % 16 || reinterpret_cast<uintptr_t>(a.base) % 16)
        return hipErrorInvalidValue;
    clear_stale_error();
    hipLaunchKernelGGL(return_plan_kernel, dim3(1), dim3(kRetThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.total_units == 0) return e;
    const dim3 grid((a.total_units + kGatherWaves - 1) / kGatherWaves, a.max_rows);
    hipLaunchKernelGGL(gather_rebuilt_kernel, grid, dim3(kGatherThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace cec
