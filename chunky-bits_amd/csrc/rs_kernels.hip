// rs_kernels.hip — gfx950 (MI355X, CDNA4) GF(2^8) Reed-Solomon kernels + synthetic fill.
//
//  rs_apply_kernel      GF(2^8) matrix x chunk-set multiply.  One kernel serves
//                       ReedSolomon::encode_sep (rows = parity rows of M, inputs = the d data
//                       chunks) and reconstruct / reconstruct_data (rows = decode rows, inputs =
//                       the first d present chunks), for thousands of parts per launch.
//                       HBM-bound: algorithmic bytes per part = (d + n_out) * len.
//  rs_apply_var_kernel  the same for a reconstruct batch whose parts miss different numbers of
//                       chunks: one launch, each block dispatched on its pattern's row count.
//  rs_apply_ragged_kernel  encode_sep for parts of different chunk lengths, one launch: one
//                       wave per 4 KiB of a part's columns, found through a prefix array.  Its
//                       SPLIT build stores the rows into a parity region of its own (the split
//                       ragged layout) through a per-part output displacement.
//  rs_reconstruct_ragged_kernel  reconstruct for such parts: a pattern record per listed part,
//                       mixed erasure counts in one launch.
//  fill_kernel          counter-based synthetic bytes for benchmarks/tests.
//
// GF multiply: no GF instruction exists, so a product c*x of four packed bytes is three
// v_perm_b32 byte-table lookups (x split into bits [2:0], [5:3], [7:6]; see gf256.hpp) combined
// with one v_bitop3_b32 (xor3).  The selectors of a data word are shared by every output row.
// Coefficient tables are wave-uniform and come in through scalar loads (s_load), so a row costs
// 3 v_perm + ~1.5 xor per data dword, with no LDS traffic and no bank conflicts.
//
// Memory shape: a block owns a 16 KiB (rs_apply_kernel) or 8 KiB (bit-sliced encoder, mixed-
// pattern reconstruct) column range of one part; each lane moves V 16-byte columns per input per
// step (V = 2: two 1 KiB-per-wave loads per input in flight) with non-temporal loads and stores
// (every byte is touched once), blocks in an XCD-aware order, and on large grids a residency cap
// of 2-3 blocks per CU (apply_lds).  RS(10,4) encode streams 6.40 TB/s and 2-erasure
// reconstruct_data 5.96 TB/s.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "device_common.hpp"
#include "gf256.hpp"
#include "gf_const.hpp"
#include "gf_device.hpp"
#include "kernels.hpp"
#include "knobs.hpp"

namespace cec {
namespace {

using namespace gf;

constexpr int kApplyThreads = 256;
constexpr uint64_t kApplyTile = 16384;  // bytes of one part's column range per block
constexpr uint64_t kSpan = uint64_t(kApplyThreads) * 16u;  // bytes per block per column step
constexpr uint32_t kMaxApplyRows = 8;

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ uint4 ld16(const uint8_t* p) {
    if (NT) {
        const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const uint4*>(p);
}

template <bool NT>
__device__ __forceinline__ void st16(uint8_t* p, uint4 v) {
    if (NT) {
        v4u w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<v4u*>(p));
    } else {
        *reinterpret_cast<uint4*>(p) = v;
    }
}

// acc[r][c] = 0 for RG rows x V 16-byte columns.
template <int RG, int V>
__device__ __forceinline__ void acc_zero(uint32_t (&acc)[RG][V][4]) {
#pragma unroll
    for (int r = 0; r < RG; ++r)
#pragma unroll
        for (int c = 0; c < V; ++c) acc[r][c][0] = acc[r][c][1] = acc[r][c][2] = acc[r][c][3] = 0u;
}

// acc[r] ^= coef[r] (x) v for one input's V columns; tj: the input's RG tables.
template <int RG, int V>
__device__ __forceinline__ void mul_input(uint32_t (&acc)[RG][V][4], const uint4 (&v)[V],
                                          cu32* tj) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const Sel s0 = selectors(v[c].x), s1 = selectors(v[c].y), s2 = selectors(v[c].z),
                  s3 = selectors(v[c].w);
#pragma unroll
        for (int r = 0; r < RG; ++r) {
            cu32* t = tj + r * kTabWords;
            const uint32_t t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];
            acc[r][c][0] ^= gmul(s0, t0, t1, t2, t3, t4);
            acc[r][c][1] ^= gmul(s1, t0, t1, t2, t3, t4);
            acc[r][c][2] ^= gmul(s2, t0, t1, t2, t3, t4);
            acc[r][c][3] ^= gmul(s3, t0, t1, t2, t3, t4);
        }
    }
}

// One row's V columns to dst (the row's chunk at the lane's first column): FULL whole 16-byte
// columns kSpan apart, else the first n bytes of the one column.
template <bool FULL, bool NT, int V>
__device__ __forceinline__ void row_store(const uint32_t (&acc)[V][4], uint8_t* dst, uint64_t n) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
        if (FULL)
            st16<NT>(dst + c * kSpan, make_uint4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]));
        else
            store_partial(dst, acc[c], n);
    }
}

// V 16-byte columns (x + c*kSpan, c < V) of a part: acc[r] = XOR_j coef[r][j] (x) in_j[...].
// FULL: every lane of the block has V*16 valid bytes and the layout is 16-byte aligned
// (otherwise V == 1 with a byte-granular load/store of a rem < 16 tail).
// p: the RG rows' view of the part's pattern record.
// GROUP inputs (x V columns) are loaded before any is multiplied; NT selects non-temporal
// loads/stores (streamed once, never re-read).  out_disp (wave-uniform) is added to every output
// address: 0 where a part's outputs lie among its inputs' chunks, the distance to the part's
// place in a parity region of its own in the split ragged layout.
template <int RG, bool FULL, int GROUP, int V, bool NT>
__device__ __forceinline__ void apply_column(uint8_t* pbase, uint64_t cs, uint64_t x,
                                             uint64_t rem, uint32_t d, const PatView& p,
                                             uint64_t out_disp = 0) {
    static_assert(FULL || V == 1, "ragged columns are single");
    uint32_t acc[RG][V][4];
    acc_zero(acc);
    const uint64_t n = rem < 16 ? rem : 16;

#pragma unroll 1
    for (uint32_t j0 = 0; j0 < d; j0 += GROUP) {
        uint4 v[GROUP][V];
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
#pragma unroll
            for (int c = 0; c < V; ++c) v[u][c] = make_uint4(0u, 0u, 0u, 0u);
            if (j0 + u < d) {
                const uint8_t* src = pbase + uint64_t(p.in_idx[j0 + u]) * cs + x;
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    if (FULL) v[u][c] = ld16<NT>(src + c * kSpan);
                    else v[u][c] = load_partial(src, n);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GROUP; ++u)
            if (j0 + u < d) mul_input(acc, v[u], p.tab + size_t(j0 + u) * p.tab_stride);
    }
#pragma unroll
    for (int r = 0; r < RG; ++r)
        row_store<FULL, NT>(acc[r], pbase + (uint64_t(p.out_idx[r]) * cs + out_disp) + x, n);
}

// The column tile `tile` (tile_bytes) of one part, RG rows: full column steps (kSpan*V bytes of an
// aligned layout, VEC) go to full(pbase, cs, x), x the lane's first column; the rest (ragged end,
// unaligned layouts) takes the byte-granular single-column path.
template <int RG, bool VEC, int V, typename Full>
__device__ __forceinline__ void walk_tile(const ApplyParams& a, uint32_t part, uint32_t tile,
                                          uint32_t tile_bytes, uint32_t d, const PatView& p,
                                          Full&& full) {
    uint8_t* pbase = a.base + uint64_t(part) * a.part_stride;
    const uint64_t len = a.len;
    const uint64_t cs = a.chunk_stride;
    const uint64_t t0 = uint64_t(tile) * tile_bytes;
    const uint64_t t1 = t0 + tile_bytes < len ? t0 + tile_bytes : len;
#pragma unroll 1
    for (uint64_t xb = t0; xb < t1; xb += kSpan * V) {  // block-uniform
        const uint64_t x = xb + uint64_t(threadIdx.x) * 16u;
        if (VEC && xb + kSpan * V <= len) {
            full(pbase, cs, x);
        } else {
#pragma unroll 1
            for (uint64_t xc = x; xc < t1 && xc < xb + kSpan * V; xc += kSpan)
                apply_column<RG, false, 4, 1, false>(pbase, cs, xc, len - xc, d, p);
        }
    }
}

// One 16 KiB column tile of one part, rows [row0, row0 + RG) of its pattern record (n_out rows
// in all).
// VEC (16-byte aligned layout): two columns per lane per step, non-temporal loads and stores;
// else one byte-granular column.  Both load 4 inputs before any is multiplied.  Measured on C2
// encode (MI355X): non-temporal 10.79 ms, plain 11.20, one column 11.25, one column
// non-temporal 11.15, groups of 8 11.26, non-temporal groups of 8 10.85.
template <int RG, bool VEC>
__device__ __forceinline__ void apply_tile(const ApplyParams& a, cu32* pat, uint32_t part,
                                           uint32_t tile, uint32_t n_out, uint32_t row0,
                                           uint32_t tile_bytes) {
    constexpr int GROUP = 4, V = VEC ? 2 : 1;
    constexpr bool NT = VEC;
    const PatView p(pat, a.d, n_out, row0);
    walk_tile<RG, VEC, V>(a, part, tile, tile_bytes, a.d, p,
                          [&](uint8_t* pbase, uint64_t cs, uint64_t x) {
        apply_column<RG, true, GROUP, V, NT>(pbase, cs, x, a.len - x, a.d, p);
    });
}

// ---- compile-time d: the same multiply with every input's loads issued one group ahead ----
// With d a run-time value the column loop above waits for each group's loads before it multiplies
// (`unroll 1`, no prefetch across groups).  For the compiled input count (rs_apply_var_kernel's
// CD = 10 builds) the loop unrolls at compile time and group J0 + G's loads go out before
// group J0's multiplies, as in the bit-sliced encoder.
template <int D, int G, int J0, int V>
__device__ __forceinline__ void vp_load(uint4 (&v)[G][V], const uint8_t* pbase, uint64_t cs,
                                        uint64_t x, cu32* in_idx) {
#pragma unroll
    for (int u = 0; u < G; ++u)
        if (J0 + u < D) {
            const uint8_t* src = pbase + uint64_t(in_idx[J0 + u]) * cs + x;
#pragma unroll
            for (int c = 0; c < V; ++c) v[u][c] = ld16<true>(src + c * kSpan);
        }
}

template <int D, int RG, int G, int J0, int V>
__device__ __forceinline__ void vp_mul(uint32_t (&acc)[RG][V][4], uint4 (&v)[G][V], cu32* tab,
                                       uint32_t tab_stride) {
#pragma unroll
    for (int u = 0; u < G; ++u)
        if (J0 + u < D) mul_input(acc, v[u], tab + size_t(J0 + u) * tab_stride);
}

template <int D, int RG, int G, int J0, int V>
struct VpSteps {
    __device__ static __forceinline__ void run(uint32_t (&acc)[RG][V][4], uint4 (&v)[2][G][V],
                                               const uint8_t* pbase, uint64_t cs, uint64_t x,
                                               cu32* in_idx, cu32* tab, uint32_t tab_stride) {
        constexpr int buf = (J0 / G) & 1;
        if constexpr (J0 + G < D) vp_load<D, G, J0 + G, V>(v[buf ^ 1], pbase, cs, x, in_idx);
        vp_mul<D, RG, G, J0, V>(acc, v[buf], tab, tab_stride);
        if constexpr (J0 + G < D)
            VpSteps<D, RG, G, J0 + G, V>::run(acc, v, pbase, cs, x, in_idx, tab, tab_stride);
    }
};

// apply_column<RG, true, ., V, true> for d == D.
template <int D, int RG, int G, int V>
__device__ __forceinline__ void vp_column(uint8_t* pbase, uint64_t cs, uint64_t x,
                                          const PatView& p) {
    uint32_t acc[RG][V][4];
    acc_zero(acc);
    uint4 v[2][G][V];
    vp_load<D, G, 0, V>(v[0], pbase, cs, x, p.in_idx);
    VpSteps<D, RG, G, 0, V>::run(acc, v, pbase, cs, x, p.in_idx, p.tab, p.tab_stride);
#pragma unroll
    for (int r = 0; r < RG; ++r)
        row_store<true, true>(acc[r], pbase + uint64_t(p.out_idx[r]) * cs + x, 16);
}

// apply_tile with d == D (aligned layout, non-temporal, two columns per lane): full steps take
// vp_column, the ragged end the byte path.
template <int D, int RG, int G>
__device__ __forceinline__ void apply_tile_cd(const ApplyParams& a, cu32* pat, uint32_t part,
                                              uint32_t tile, uint32_t n_out, uint32_t tile_bytes) {
    constexpr int V = 2;
    const PatView p(pat, D, n_out);
    walk_tile<RG, true, V>(a, part, tile, tile_bytes, D, p,
                           [&](uint8_t* pbase, uint64_t cs, uint64_t x) {
        vp_column<D, RG, G, V>(pbase, cs, x, p);
    });
}

// XCD-aware block order.  The dispatcher deals a grid's blocks to the 8 XCDs round-robin (block
// b to XCD b % 8), so in launch order neighbouring tiles of a part land on different XCDs and
// every XCD streams a slice of every part at once.  Renumbering so that XCD x runs the contiguous
// range [x*q + min(x, r), ...) of the n blocks (q = n / 8, r = n % 8: a bijection for any n)
// gives each XCD whole runs of parts instead.  For the 10-read / 4-write stream of an RS(10,4)
// encode with no GF work this lifts the chip from 5.72-5.74 to 6.26-6.27 TB/s
// (tools/ubench_stream.hip mode m, profiles/r3_full/ubench_mix.log).
constexpr uint32_t kXcds = 8;

__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t n) {
    const uint32_t x = b % kXcds, i = b / kXcds, q = n / kXcds, r = n % kXcds;
    return x * q + (x < r ? x : r) + i;
}

// This block's listed part and column tile of it (grid.x = listed parts * tiles_per_part).  xcd:
// block order of xcd_block (else launch order).
struct BlockTile {
    uint32_t lp, tile;
};
__device__ __forceinline__ BlockTile block_tile(uint32_t tiles_per_part, bool xcd) {
    const uint32_t bx = xcd ? xcd_block(blockIdx.x, gridDim.x) : blockIdx.x;
    const uint32_t lp = bx / tiles_per_part;
    return {lp, bx - lp * tiles_per_part};
}

// grid.x = n_parts * tiles_per_part (one 16 KiB column tile of one part per block),
// grid.y = row groups of exactly RG output rows starting at row_base.
template <int RG, bool VEC>
__global__ __launch_bounds__(kApplyThreads) void rs_apply_kernel(ApplyParams a,
                                                                 uint32_t tiles_per_part,
                                                                 uint32_t row_base, bool xcd,
                                                                 uint32_t tile_bytes) {
    const BlockTile b = block_tile(tiles_per_part, xcd);
    const uint32_t part = a.part_ids ? as_const(a.part_ids)[b.lp] : b.lp;
    cu32* pat = as_const(a.pat) + (a.part_pat ? as_const(a.part_pat)[b.lp] : 0u);
    apply_tile<RG, VEC>(a, pat, part, b.tile, a.n_rows, row_base + blockIdx.y * RG, tile_bytes);
}

// Reconstruct with mixed erasure counts in ONE launch: every listed part's pattern carries its
// own row count n_out (1..MAXRG, the record's first word); each block branches (block-uniformly)
// to the exact-RG body, so no row is predicated inside the inner loop.  MAXRG is the batch's
// largest row count rounded up to 2, 4 or 8 (host side): the kernel's register allocation is the
// widest body's, so a 2-erasure batch compiled for 8 rows would run at half the occupancy.
// CD > 0 (aligned builds only): the batch's d equals CD (host-checked), every tile takes
// apply_tile_cd with loads kCdGroup inputs ahead.  Interleaved on one box with the residency
// caps (profiles/r3_cap_ab/), against the run-time-d kernel: c3e2 8.07-8.09 vs 8.12-8.14 ms,
// C3 9.64-9.68 vs 9.71-9.75 (groups of 2 and 10 measured the same as 5 without the caps,
// profiles/r3_cd_ab/).
constexpr int kCdGroup = 5;

template <int RG, int MAXRG, typename F>
__host__ __device__ __forceinline__ void rg_dispatch(uint32_t n, F&& f) {
    if (n == RG) f(std::integral_constant<int, RG>{});
    else if constexpr (RG < MAXRG) rg_dispatch<RG + 1, MAXRG>(n, f);
    // n > MAXRG or 0: never listed -- the host routes n_out > 8 to row-group launches and checks
    // every listed record against the launch's row class (capi.cpp reconstruct_batch)
}

template <bool VEC, int MAXRG, int CD = 0>
__global__ __launch_bounds__(kApplyThreads) void rs_apply_var_kernel(ApplyParams a,
                                                                     uint32_t tiles_per_part,
                                                                     bool xcd, uint32_t tile_bytes) {
    const BlockTile b = block_tile(tiles_per_part, xcd);
    const uint32_t part = as_const(a.part_ids)[b.lp];
    cu32* pat = as_const(a.pat) + as_const(a.part_pat)[b.lp];
    rg_dispatch<1, MAXRG>(pat[0], [&](auto rg) {
        constexpr int RG = decltype(rg)::value;
        if constexpr (CD > 0) {
            static_assert(VEC, "compile-time d: aligned build");
            apply_tile_cd<CD, RG, kCdGroup>(a, pat, part, b.tile, RG, tile_bytes);
        } else {
            apply_tile<RG, VEC>(a, pat, part, b.tile, RG, 0, tile_bytes);
        }
    });
}

// ------------------------------------------------------------------------------------------
// Ragged batch: parts whose chunk lengths differ, one launch.
//
// Part k's chunk i is at base + off[k] + i * stride(L_k), stride(L) = L rounded up to 16, base and
// off[k] multiples of 16: every chunk starts 16-byte aligned and only its last column is partial.
// The work unit is one WAVE's kRaggedUnit (4 KiB) column range of one part: a wave finds its
// part with a binary search over the host-built prefix array of units (scalar loads, the wave
// number made uniform with readfirstlane), then walks its unit in 1 KiB steps (64 lanes x one
// 16-byte column) through apply_column.  The four waves of a workgroup are independent, so a
// batch of thousands of sub-kilobyte parts spends one wave per part, and a 1 MiB chunk is 256
// units that stream full 16-byte columns whatever the lengths of its neighbours.  Only the last
// step of a part diverges: lanes with a whole column take the vector path, the one lane with the
// chunk's last 1..15 bytes the byte path, lanes past the end nothing.
// Plain (not non-temporal) loads: the SHA-256 launch behind it reads the same chunks again.
// ------------------------------------------------------------------------------------------
constexpr uint64_t kRaggedUnit = 4096;                  // bytes of one chunk's columns per wave
constexpr uint64_t kRaggedStep = 64u * 16u;             // bytes per wave per column step
constexpr uint32_t kRaggedWaves = kApplyThreads / 64;   // units per workgroup

// Work unit u < a.total_units: the listed part that owns it, pre[lp] <= u < pre[lp + 1] (wave-
// uniform scalar loads), and the unit's first column in it.
struct WaveUnit {
    uint32_t lp;
    uint64_t x0;
};
__device__ __forceinline__ WaveUnit wave_unit(const RaggedParams& a, uint32_t u) {
    cu32* pre = as_const(a.units);
    uint32_t lo = 0, hi = a.n_parts;  // pre[lo] <= u < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= u) lo = mid;
        else hi = mid;
    }
    return {lo, uint64_t(u - pre[lo]) * kRaggedUnit};
}

// One 4 KiB unit (columns from x0) of the part described by pm = {off lo, off hi, L lo, L hi}:
// rows [row0, row0 + RG) of the record `pat`, n_out rows in all.  SPLIT: pm carries two more
// words {disp lo, disp hi}, the part's output displacement (apply_column; scalar like the rest of
// the record), so the rows land in the parity region and nothing is stored among the inputs.
template <int RG, bool SPLIT = false>
__device__ __forceinline__ void ragged_unit(uint8_t* base, cu32* pm, uint64_t x0, uint32_t d,
                                            cu32* pat, uint32_t n_out, uint32_t row0) {
    const uint64_t off = uint64_t(pm[0]) | (uint64_t(pm[1]) << 32);
    const uint64_t len = uint64_t(pm[2]) | (uint64_t(pm[3]) << 32);
    const uint64_t disp = SPLIT ? uint64_t(pm[4]) | (uint64_t(pm[5]) << 32) : 0;
    const uint64_t cs = (len + 15) & ~uint64_t(15);
    uint8_t* pbase = base + off;
    const PatView p(pat, d, n_out, row0);
    const uint64_t x1 = x0 + kRaggedUnit < len ? x0 + kRaggedUnit : len;
    const uint64_t lane_x = uint64_t(threadIdx.x & 63u) * 16u;
#pragma unroll 1
    for (uint64_t xb = x0; xb < x1; xb += kRaggedStep) {  // wave-uniform
        const uint64_t x = xb + lane_x;
        if (x + 16 <= len) {  // every lane of a step that is not the part's last
            apply_column<RG, true, 4, 1, false>(pbase, cs, x, len - x, d, p, disp);
        } else if (x < len) {
            apply_column<RG, false, 4, 1, false>(pbase, cs, x, len - x, d, p, disp);
        }
    }
}

// grid.x = ceil(total_units / kRaggedWaves), grid.y = row groups of exactly RG rows from row_base.
// Every listed part uses the record at pat + part_pat[lp] (null: the one record at pat, the
// encode), all of a.n_rows rows.  SPLIT: the split layout's six-word part records (a.split).
template <int RG, bool SPLIT = false>
__global__ __launch_bounds__(kApplyThreads) void rs_apply_ragged_kernel(RaggedParams a,
                                                                        uint32_t row_base) {
    const uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * kRaggedWaves +
                                                      (threadIdx.x >> 6));
    if (u >= a.total_units) return;  // wave-uniform
    const WaveUnit w = wave_unit(a, u);
    cu32* pat = as_const(a.pat) + (a.part_pat ? as_const(a.part_pat)[w.lp] : 0u);
    ragged_unit<RG, SPLIT>(a.base, as_const(a.parts) + size_t(w.lp) * (SPLIT ? 6 : 4), w.x0, a.d,
                           pat, a.n_rows, row_base + blockIdx.y * RG);
}

// Ragged reconstruct: the listed parts are the ones that need a rebuild, each
// with its own pattern record at pat + part_pat[lp] (inputs = its first d present chunks, outputs
// = its missing chunks), so parts that miss different numbers of chunks share ONE launch.  The
// wave reads its record's row count (word 0: a scalar load, wave-uniform) and branches to the
// exact-RG body as rs_apply_var_kernel does per block; MAXRG is the row class (2, 4 or 8) the
// host picked from the widest listed record, and a record outside 1..MAXRG writes nothing (the
// host refuses such a list before launching).  Exactly L_k bytes of each rebuilt chunk are
// written: present chunks, the padding up to the stride and unlisted parts are never stored to.
// Plain loads, as the encode (the verification in front of it has just read the same chunks), and
// plain stores: what is rebuilt is read next, by the copy back to the host or the caller's
// consumer, and nothing here streams far enough past the L2 for a non-temporal hint to matter.
template <int MAXRG>
__global__ __launch_bounds__(kApplyThreads) void rs_reconstruct_ragged_kernel(RaggedParams a) {
    const uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * kRaggedWaves +
                                                      (threadIdx.x >> 6));
    if (u >= a.total_units) return;  // wave-uniform
    const WaveUnit w = wave_unit(a, u);
    cu32* pat = as_const(a.pat) + as_const(a.part_pat)[w.lp];
    cu32* pm = as_const(a.parts) + size_t(w.lp) * 4;
    rg_dispatch<1, MAXRG>(pat[0], [&](auto rg) {
        constexpr int RG = decltype(rg)::value;
        ragged_unit<RG>(a.base, pm, w.x0, a.d, pat, RG, 0);
    });
}

// ------------------------------------------------------------------------------------------
// Bit-sliced encode for the common shapes: RS(d, p) with the parity rows compile-time constants.
//
// The v_perm multiply above costs, per data dword, 3 selector ops plus 3 half-rate v_perm and
// 2 xors per parity row: for RS(10,4) about 84 SIMD cycles per 64 data dwords, against ~39 for
// the HBM stream (the encode was co-bound).  Bit-sliced, the same multiply is a
// fixed XOR network: a lane's 32 bytes of one input (its two 16-byte columns) are transposed
// into 8 bit planes (plane i = bit i of all 32 bytes; 12 two-word bit swaps, 48 full-rate ops),
// output plane o of row r is the XOR of the input planes i with bit o of c[r][j]*2^i set
// (gf_const.hpp kBits, about half of them), and the 8 planes of each row are transposed back.
// With the matrix known at compile time the network is straight-line v_bitop3 xor3s: RS(10,4)
// ≈ 17 full-rate ops per data dword (6 transpose in, 9 xor, 2.4 transpose out), about half the
// v_perm form.  Loads and stores are the rs_apply ones (non-temporal, two 16-byte columns 4 KiB
// apart per lane, XCD-aware block order); ragged tails take the v_perm byte path.
// ------------------------------------------------------------------------------------------

// bitop3 select: m ? x : y per bit.
__device__ __forceinline__ uint32_t bsel(uint32_t m, uint32_t x, uint32_t y) {
    return __builtin_amdgcn_bitop3_b32(m, x, y, 0xCA);
}

// Swap bit k (k & S set) of a with bit k - S of b, in every byte.
template <int S>
__device__ __forceinline__ void swap_bits(uint32_t& a, uint32_t& b) {
    constexpr uint32_t lo = S == 1 ? 0x55555555u : S == 2 ? 0x33333333u : 0x0F0F0F0Fu;
    constexpr uint32_t hi = lo << S;
    const uint32_t na = bsel(hi, b << S, a);
    const uint32_t nb = bsel(lo, a >> S, b);
    a = na;
    b = nb;
}

// 8x8 bit transpose in each byte lane of 8 words: bit k of byte m of w[j] <-> bit j of byte m of
// w[k].  Each stage swaps one bit of the word index with the same bit of the bit index, so the
// three commute and the whole is an involution (the same network maps planes back to bytes).
__device__ __forceinline__ void transpose8(uint32_t (&w)[8]) {
    swap_bits<1>(w[0], w[1]);
    swap_bits<1>(w[2], w[3]);
    swap_bits<1>(w[4], w[5]);
    swap_bits<1>(w[6], w[7]);
    swap_bits<2>(w[0], w[2]);
    swap_bits<2>(w[1], w[3]);
    swap_bits<2>(w[4], w[6]);
    swap_bits<2>(w[5], w[7]);
    swap_bits<4>(w[0], w[4]);
    swap_bits<4>(w[1], w[5]);
    swap_bits<4>(w[2], w[6]);
    swap_bits<4>(w[3], w[7]);
}

constexpr int kBsGroup = 2;  // inputs per network step (terms pair across both into xor3s)

// Input words of inputs J0 .. J0 + kBsGroup: a lane's two 16-byte columns (x, x + kSpan).
template <int D, int J0>
__device__ __forceinline__ void bs_load(uint32_t (&w)[kBsGroup][8], const uint8_t* pbase,
                                        uint64_t cs, uint64_t x, cu32* in_idx) {
#pragma unroll
    for (int u = 0; u < kBsGroup; ++u) {
        if (J0 + u < D) {
            const uint8_t* src = pbase + uint64_t(in_idx[J0 + u]) * cs + x;
            const uint4 c0 = ld16<true>(src), c1 = ld16<true>(src + kSpan);
            w[u][0] = c0.x, w[u][1] = c0.y, w[u][2] = c0.z, w[u][3] = c0.w;
            w[u][4] = c1.x, w[u][5] = c1.y, w[u][6] = c1.z, w[u][7] = c1.w;
        }
    }
}

// acc[r][o] ^= the planes of inputs J0 .. J0 + kBsGroup that feed bit o of row r, two per xor3.
template <int D, int P, int J0>
__device__ __forceinline__ void bs_group(uint32_t (&acc)[P][8], uint32_t (&w)[kBsGroup][8]) {
    using S = gfc::Shape<D, P>;
#pragma unroll
    for (int u = 0; u < kBsGroup; ++u)
        if (J0 + u < D) transpose8(w[u]);
#pragma unroll
    for (int r = 0; r < P; ++r) {
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            uint32_t pend = 0;
            bool has = false;
#pragma unroll
            for (int u = 0; u < kBsGroup; ++u) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (J0 + u < D && ((S::kBits.m[r][J0 + u < D ? J0 + u : 0][o] >> i) & 1)) {
                        if (has) {
                            acc[r][o] = xor3(acc[r][o], pend, w[u][i]);
                            has = false;
                        } else {
                            pend = w[u][i];
                            has = true;
                        }
                    }
                }
            }
            if (has) acc[r][o] ^= pend;
        }
    }
}

// Groups J0, J0 + kBsGroup, ... with the next group's loads issued before this group's network.
template <int D, int P, int J0>
struct BsSteps {
    __device__ static __forceinline__ void run(uint32_t (&acc)[P][8],
                                               uint32_t (&w)[2][kBsGroup][8],
                                               const uint8_t* pbase, uint64_t cs, uint64_t x,
                                               cu32* in_idx) {
        constexpr int buf = (J0 / kBsGroup) & 1;
        if constexpr (J0 + kBsGroup < D) bs_load<D, J0 + kBsGroup>(w[buf ^ 1], pbase, cs, x, in_idx);
        bs_group<D, P, J0>(acc, w[buf]);
        if constexpr (J0 + kBsGroup < D)
            BsSteps<D, P, J0 + kBsGroup>::run(acc, w, pbase, cs, x, in_idx);
    }
};

// Two full 16-byte columns (x, x + kSpan) of every parity row of one part.
template <int D, int P>
__device__ __forceinline__ void bs_column(uint8_t* pbase, uint64_t cs, uint64_t x, cu32* in_idx,
                                          cu32* out_idx) {
    uint32_t acc[P][8];
#pragma unroll
    for (int r = 0; r < P; ++r)
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[r][o] = 0u;
    uint32_t w[2][kBsGroup][8];
    bs_load<D, 0>(w[0], pbase, cs, x, in_idx);
    BsSteps<D, P, 0>::run(acc, w, pbase, cs, x, in_idx);
#pragma unroll
    for (int r = 0; r < P; ++r) {
        transpose8(acc[r]);
        uint8_t* dst = pbase + uint64_t(out_idx[r]) * cs + x;
        st16<true>(dst, make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]));
        st16<true>(dst + kSpan, make_uint4(acc[r][4], acc[r][5], acc[r][6], acc[r][7]));
    }
}

// grid.x = n_parts * tiles_per_part, as rs_apply_kernel; the pattern record is the codec's
// encode record (its indices; its v_perm tables serve the ragged tail).  The host launches this
// only for 16-byte aligned layouts whose run-time matrix equals gfc::Shape<D, P> (checked once
// per codec, bs_encode_matches).
template <int D, int P>
__global__ __launch_bounds__(kApplyThreads) void rs_encode_bs_kernel(ApplyParams a,
                                                                     uint32_t tiles_per_part,
                                                                     bool xcd, uint32_t tile_bytes) {
    const BlockTile b = block_tile(tiles_per_part, xcd);
    const uint32_t part = a.part_ids ? as_const(a.part_ids)[b.lp] : b.lp;
    const PatView p(as_const(a.pat), D, P);
    walk_tile<P, true, 2>(a, part, b.tile, tile_bytes, D, p,
                          [&](uint8_t* pbase, uint64_t cs, uint64_t x) {
        bs_column<D, P>(pbase, cs, x, p.in_idx, p.out_idx);
    });
}

// ------------------------------------------------------------------------------------------
// Synthetic data
// ------------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__host__ __device__ __forceinline__ uint64_t synth_key(uint64_t seed, uint64_t part,
                                                       uint64_t chunk) {
    return mix64(seed ^ mix64(part * 0x100000001B3ull + chunk + 0x9E3779B97F4A7C15ull));
}

__host__ __device__ __forceinline__ uint64_t synth_word(uint64_t key, uint64_t word) {
    return mix64(key + word * 0x9E3779B97F4A7C15ull);
}

__global__ __launch_bounds__(256) void fill_kernel(FillParams a, bool aligned8) {
    const uint64_t words = (a.len + 7) / 8;
    const uint64_t n_inst = uint64_t(a.n_parts) * a.n_chunks;
    for (uint64_t inst = blockIdx.y; inst < n_inst; inst += gridDim.y) {
        const uint64_t k = inst / a.n_chunks;
        const uint64_t c = inst - k * a.n_chunks;
        const uint64_t key = synth_key(a.seed, k, c);
        uint8_t* dst = a.base + k * a.part_stride + c * a.chunk_stride;
        for (uint64_t w = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < words;
             w += uint64_t(gridDim.x) * blockDim.x) {
            const uint64_t v = synth_word(key, w);
            const uint64_t off = w * 8;
            if (aligned8 && off + 8 <= a.len) {
                *reinterpret_cast<uint64_t*>(dst + off) = v;
            } else {
                for (int b = 0; b < 8; ++b)
                    if (off + b < a.len) dst[off + b] = uint8_t(v >> (8 * b));
            }
        }
    }
}

// LDS of one CU on the current device, cached per device: 160 KiB on gfx950 (MI355X), else
// what the runtime reports (hipDeviceAttributeMaxSharedMemoryPerMultiprocessor); 0 when
// unknown, which turns the residency caps below off rather than mis-sizing them.
uint32_t lds_per_cu() {
    static std::atomic<uint32_t> cache[kMaxDevices];  // 0 = not read yet, 1 = unknown
    const uint32_t v = per_device(cache, 1u, [](int dev) {
        hipDeviceProp_t prop;
        int attr = 0;
        uint32_t lds = 1;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess &&
            std::strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            lds = kCuLdsBytes;
        else if (hipDeviceGetAttribute(&attr, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor,
                                       dev) == hipSuccess && attr > 0)
            lds = uint32_t(attr);
        clear_stale_error();
        return lds;
    });
    return v == 1 ? 0 : v;
}

// Residency cap.  The GF kernels stream 10-28 chunks per part 1 MiB (chunk stride) apart, and on
// MI355X they run faster with FEWER blocks in flight than their registers allow: interleaved on
// one box (profiles/r3_occ_ab/), RS(10,4) bit-sliced encode 9.53 ms at 2 blocks (= waves per
// SIMD) per CU vs 9.88 at its register-bound 6; 2-erasure reconstruct_data 8.11 at 2 vs 8.26 at
// 3 (the 8-row build) and 8.57 at 6 (the 2-row build); C3 (1-4 rows) 9.58 at 3 vs 10.15 at 2;
// RS(20,8) encode no different (3 by registers).  The cap is an unused LDS reservation (160 KiB
// per CU), on top of any the caller asked for, and only for grids of at least kCapMinBlocks
// blocks (the device-resident batches it was measured on; the host pipelines' 256-part batches
// share the chip with SHA-256 kernels and keep the register-bound occupancy).  `cap` is the
// launching kernel's measured blocks per CU (0 = none).
constexpr uint64_t kCapMinBlocks = 65536;
uint32_t apply_lds(uint32_t reserve, int cap, uint64_t n_blocks) {
    const int n = n_blocks >= kCapMinBlocks ? cap : 0;
    const uint32_t cu_lds = lds_per_cu();
    if (n <= 0 || n > 16 || cu_lds == 0) return reserve;
    // floor(cu_lds / lds) == n; a cap the part's LDS cannot express (lds above the per-launch
    // maximum, 64 KiB parts at n = 1) is dropped rather than failing the launch
    const uint32_t lds = cu_lds / uint32_t(n + 1) + 2048u;
    if (lds > cu_lds) return reserve;
    return std::max(reserve, lds);
}

// Bytes of one part's column range per block (a kernel argument): kApplyTile for
// rs_apply_kernel, kBsTile for the bit-sliced encoder and the mixed-pattern reconstruct.
// Measured interleaved on one box with the residency caps (profiles/r3_tilecap_ab/, 8 / 16 /
// 32 KiB): RS(10,4) bit-sliced encode 9.46 / 9.72 / 9.86 ms, c3e2 7.89 / 7.96 / 8.39, C3 9.20 /
// 9.35 / 9.61.  (Without the caps C3 had preferred 16 KiB, profiles/r3_tile2_ab/.)
constexpr uint64_t kBsTile = 8192;

// Lets `kernel` reserve `bytes` of dynamic LDS (a host-side attribute; set on every such launch,
// since the instantiations share one function-pointer type).
template <typename K>
bool allow_lds(K kernel, uint32_t bytes) {
    return bytes <= 64 * 1024 ||
           hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes)) == hipSuccess;
}

// A dispatch's grid is at most 2^32 - 1 work-items (the AQL packet's 32-bit grid size): with
// kApplyThreads per block, at most this many blocks.  Larger batches (many parts of long chunks,
// e.g. 4096 x 64 MiB) are split over several launches of whole parts.
constexpr uint64_t kMaxApplyBlocks = 0xFFFFFFFFull / kApplyThreads;
// CEC_APPLY_MAX_BLOCKS (test knob) lowers the limit so the split is exercised
// at test sizes; results are identical either way.
uint64_t max_apply_blocks() {
    const uint64_t v = knobs().apply_max_blocks;
    return v ? std::min<uint64_t>(v, kMaxApplyBlocks) : kMaxApplyBlocks;
}

// fn(sub) for launches of at most max_parts parts each: part ranges [p0, p0 + n) as a base
// offset (parts addressed directly) or as offsets into the listed part_ids / part_pat.
template <typename Fn>
hipError_t for_part_ranges(const ApplyParams& a, uint64_t max_parts, Fn fn) {
    for (uint64_t p0 = 0; p0 < a.n_parts; p0 += max_parts) {
        ApplyParams b = a;
        b.n_parts = uint32_t(std::min<uint64_t>(max_parts, a.n_parts - p0));
        if (a.part_ids) {
            b.part_ids = a.part_ids + p0;
            if (a.part_pat) b.part_pat = a.part_pat + p0;
        } else {
            b.base = a.base + p0 * a.part_stride;
        }
        const hipError_t e = fn(b);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One launch per part range of `kern` over tiles of tb bytes: grid.x = listed parts * tiles,
// grid.y = groups, at most `cap` blocks per CU (apply_lds); the kernel's arguments are the range's
// ApplyParams, the tiles per part, `extra`, the XCD order and tb.
template <typename K, typename... Extra>
hipError_t launch_tiled(const ApplyParams& a, K kern, uint64_t tb, uint32_t groups, int cap,
                        hipStream_t s, Extra... extra) {
    const uint64_t tiles = (a.len + tb - 1) / tb;
    const uint64_t max_blocks = max_apply_blocks();
    if (tiles > max_blocks) return hipErrorInvalidValue;
    return for_part_ranges(a, max_blocks / tiles, [&](const ApplyParams& b) {
        const dim3 grid(uint32_t(b.n_parts * tiles), groups);
        const uint32_t lds = apply_lds(b.lds_reserve, cap, uint64_t(grid.x) * groups);
        if (!allow_lds(kern, lds)) return hipErrorInvalidValue;
        clear_stale_error();
        hipLaunchKernelGGL(kern, grid, dim3(kApplyThreads), lds, s, b, uint32_t(tiles), extra...,
                           /*xcd=*/true, uint32_t(tb));
        return hipGetLastError();
    });
}

template <int RG>
hipError_t launch_rg(const ApplyParams& a, uint32_t row_base, uint32_t groups, bool vec16,
                     hipStream_t s) {
    // layouts that are not 16-byte aligned take the byte-granular build
    auto* kern = vec16 ? &rs_apply_kernel<RG, true> : &rs_apply_kernel<RG, false>;
    // 1-3 rows: 3 blocks per CU (RS(2,1) / RS(4,2) / RS(8,2) / RS(6,3) encode 1-2 %
    // faster than by registers, profiles/r3_vperm_shapes_ab/); 4+ rows: no gain
    return launch_tiled(a, kern, kApplyTile, groups, RG <= 3 ? 3 : 0, s, row_base);
}

// Rows are processed in groups of kMaxApplyRows (8) plus one remainder group, so every kernel
// instance handles exactly RG rows (no per-row predicate in the inner loop):
// fn(std::integral_constant<int, RG>, row_base, groups) per launch.
template <typename Fn>
hipError_t for_row_groups(uint32_t n_rows, Fn fn) {
    const uint32_t full = n_rows / kMaxApplyRows, rem = n_rows % kMaxApplyRows;
    hipError_t e = hipSuccess;
    if (full) e = fn(std::integral_constant<int, int(kMaxApplyRows)>{}, 0u, full);
    if (rem && e == hipSuccess)
        rg_dispatch<1, kMaxApplyRows - 1>(rem, [&](auto rg) {
            e = fn(rg, full * kMaxApplyRows, 1u);
        });
    return e;
}

// The row class (MAXRG: 2, 4 or 8) of a launch whose widest record has `rows` rows (0: unknown,
// the 8-row class): fn(std::integral_constant<int, MAXRG>).
template <typename Fn>
hipError_t with_row_class(uint32_t rows, Fn fn) {
    if (rows && rows <= 2) return fn(std::integral_constant<int, 2>{});
    if (rows && rows <= 4) return fn(std::integral_constant<int, 4>{});
    return fn(std::integral_constant<int, 8>{});
}

// CEC_APPLY_BS (test knob; unset = 1): 0 sends the compiled shapes' encodes to
// the v_perm kernel too.
bool apply_bs() { return knobs().apply_bs; }

template <int D, int P>
hipError_t launch_bs(const ApplyParams& a, hipStream_t s) {
    // measured per shape: RS(10,4) 2 blocks per CU, RS(3,2) 3 (6.71 vs 6.92-7.23 ms for 8 192
    // parts x 1 MiB, profiles/r3_c1enc_ab/), RS(20,8) its register-bound 3
    const int cap = D == 10 && P == 4 ? 2 : D == 3 && P == 2 ? 3 : 0;
    return launch_tiled(a, &rs_encode_bs_kernel<D, P>, kBsTile, 1, cap, s);
}

// The compiled bit-sliced shapes: the reference's example clusters (RS(3,2), examples/*.yaml)
// and the bench configurations (RS(10,4), RS(20,8)).
template <typename Fn>
bool with_bs_shape(uint32_t d, uint32_t p, Fn&& fn) {
    if (d == 3 && p == 2) return fn(gfc::Shape<3, 2>{}, std::integral_constant<int, 3>{},
                                    std::integral_constant<int, 2>{});
    if (d == 10 && p == 4) return fn(gfc::Shape<10, 4>{}, std::integral_constant<int, 10>{},
                                     std::integral_constant<int, 4>{});
    if (d == 20 && p == 8) return fn(gfc::Shape<20, 8>{}, std::integral_constant<int, 20>{},
                                     std::integral_constant<int, 8>{});
    return false;
}

}  // namespace

bool bs_encode_matches(uint32_t d, uint32_t p, const uint8_t* parity_rows) {
    return with_bs_shape(d, p, [&](auto shape, auto, auto) {
        using S = decltype(shape);
        for (uint32_t r = 0; r < p; ++r)
            for (uint32_t j = 0; j < d; ++j)
                if (S::kMat.c[r][j] != parity_rows[r * d + j]) return false;
        return true;
    });
}

hipError_t launch_rs_encode(const ApplyParams& a, bool vec16, hipStream_t s) {
    if (a.n_parts == 0 || a.n_rows == 0 || a.len == 0) return hipSuccess;
    if (a.std_encode && vec16 && !a.part_pat && apply_bs()) {
        hipError_t e = hipErrorInvalidValue;
        const bool shaped = with_bs_shape(a.d, a.n_rows, [&](auto, auto dd, auto pp) {
            e = launch_bs<decltype(dd)::value, decltype(pp)::value>(a, s);
            return true;
        });
        if (shaped) return e;
    }
    return launch_rs_apply(a, vec16, s);
}

hipError_t launch_rs_apply(const ApplyParams& a, bool vec16, hipStream_t s) {
    if (a.n_parts == 0 || a.n_rows == 0 || a.len == 0) return hipSuccess;
    return for_row_groups(a.n_rows, [&](auto rg, uint32_t row_base, uint32_t groups) {
        return launch_rg<decltype(rg)::value>(a, row_base, groups, vec16, s);
    });
}

// Listed parts (part_ids / part_pat) whose patterns have 1..kMaxApplyRows rows each: one launch.
// a.n_rows = the largest row count in the batch (0: unknown, up to kMaxApplyRows).
hipError_t launch_rs_apply_var(const ApplyParams& a, bool vec16, hipStream_t s) {
    if (a.n_parts == 0 || a.len == 0) return hipSuccess;
    if (!a.part_ids || !a.part_pat) return hipErrorInvalidValue;
    if (a.n_rows > kMaxApplyRows) return hipErrorInvalidValue;
    // not under a caller's LDS reservation: the read path's decode beside the SHA-256
    // verification (capi.cpp kDecodeLds) loses with it (c3r 44.0-44.5 vs 42.6-42.8 ms,
    // profiles/r3_c3r_ab/): its loads run ahead into the SHA chains' bandwidth
    const bool cd = a.lds_reserve == 0;
    return with_row_class(a.n_rows, [&](auto cls) {
        constexpr int MAXRG = decltype(cls)::value;
        auto* kern = !vec16             ? &rs_apply_var_kernel<false, MAXRG>
                     : a.d == 10 && cd ? &rs_apply_var_kernel<true, MAXRG, 10>
                                       : &rs_apply_var_kernel<true, MAXRG>;
        // 8 KiB tiles with the caps (see kBsTile); 2-row class: 2 blocks per CU, 4-row class: 3,
        // 8-row: by registers (3)
        return launch_tiled(a, kern, kBsTile, 1, MAXRG == 2 ? 2 : MAXRG == 4 ? 3 : 0, s);
    });
}

uint32_t max_var_rows() { return kMaxApplyRows; }

uint64_t ragged_unit_bytes() { return kRaggedUnit; }
uint64_t ragged_max_units() { return kMaxApplyBlocks * kRaggedWaves; }

namespace {

template <int RG>
hipError_t launch_ragged_rg(const RaggedParams& a, uint32_t row_base, uint32_t groups,
                            hipStream_t s) {
    const dim3 grid((a.total_units + kRaggedWaves - 1) / kRaggedWaves, groups);
    clear_stale_error();
    if (a.split)
        hipLaunchKernelGGL((rs_apply_ragged_kernel<RG, true>), grid, dim3(kApplyThreads), 0, s, a,
                           row_base);
    else
        hipLaunchKernelGGL(rs_apply_ragged_kernel<RG>, grid, dim3(kApplyThreads), 0, s, a, row_base);
    return hipGetLastError();
}

}  // namespace

// Row groups as launch_rs_apply: up to kMaxApplyRows rows (every compiled shape) is one launch.
hipError_t launch_rs_encode_ragged(const RaggedParams& a, hipStream_t s) {
    if (a.n_parts == 0 || a.n_rows == 0 || a.total_units == 0) return hipSuccess;
    if (a.total_units > ragged_max_units()) return hipErrorInvalidValue;
    return for_row_groups(a.n_rows, [&](auto rg, uint32_t row_base, uint32_t groups) {
        return launch_ragged_rg<decltype(rg)::value>(a, row_base, groups, s);
    });
}

// Listed parts with a record each of 1..kMaxApplyRows rows: one launch, in the row class of
// a.n_rows (the widest listed record; 0 = unknown, the 8-row class).
hipError_t launch_rs_reconstruct_ragged(const RaggedParams& a, hipStream_t s) {
    if (a.n_parts == 0 || a.total_units == 0) return hipSuccess;
    if (!a.part_pat || a.split || a.n_rows > kMaxApplyRows) return hipErrorInvalidValue;
    if (a.total_units > ragged_max_units()) return hipErrorInvalidValue;
    const dim3 grid((a.total_units + kRaggedWaves - 1) / kRaggedWaves);
    clear_stale_error();
    return with_row_class(a.n_rows, [&](auto cls) {
        hipLaunchKernelGGL(rs_reconstruct_ragged_kernel<decltype(cls)::value>, grid,
                           dim3(kApplyThreads), 0, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_fill(const FillParams& a, hipStream_t s) {
    const uint64_t n_inst = uint64_t(a.n_parts) * a.n_chunks;
    if (n_inst == 0 || a.len == 0) return hipSuccess;
    const uint64_t words = (a.len + 7) / 8;
    uint32_t gx = uint32_t(std::min<uint64_t>((words + 255) / 256, 64));
    uint32_t gy = uint32_t(std::min<uint64_t>(n_inst, 65535));
    const bool aligned8 = (reinterpret_cast<uintptr_t>(a.base) % 8 == 0) &&
                          (a.part_stride % 8 == 0) && (a.chunk_stride % 8 == 0);
    clear_stale_error();
    hipLaunchKernelGGL(fill_kernel, dim3(gx, gy), dim3(256), 0, s, a, aligned8);
    return hipGetLastError();
}

uint8_t synth_byte(uint64_t seed, uint64_t part, uint64_t chunk, uint64_t offset) {
    const uint64_t v = synth_word(synth_key(seed, part, chunk), offset / 8);
    return uint8_t(v >> (8 * (offset % 8)));
}

}  // namespace cec
