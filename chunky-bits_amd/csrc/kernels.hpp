// kernels.hpp — launch interface of the gfx950 kernels (kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace cec {

// One launch of the GF(2^8) matrix-apply kernel over a set of parts that share the output-row
// count.  Part `lp` of the launch is batch part part_ids[lp] (or lp), uses the pattern record at
// pat + part_pat[lp] (or pat + 0); see gf256.hpp for the record layout.  For each part:
//   chunk[out_idx[r]] = XOR_j coef[r][j] (x) chunk[in_idx[j]]     (bytes [0, len))
struct ApplyParams {
    uint8_t* base;
    uint64_t part_stride;
    uint64_t chunk_stride;
    uint64_t len;
    const uint32_t* pat;
    const uint32_t* part_ids;
    const uint32_t* part_pat;
    uint32_t n_parts;
    uint32_t d;
    uint32_t n_rows;  // n_out shared by every pattern of this launch (var launch: the largest)
    // Dynamic LDS each workgroup reserves (never touched; 0 = none).  Above 64 KiB a block
    // cannot share a CU with a SHA-256 lane-kernel workgroup (>= 64 KiB reserved each), which
    // keeps a decode running beside a verification off the SHA waves' SIMDs.
    uint32_t lds_reserve;
    // Nonzero: `pat` is the codec's encode record (inputs 0..d-1, outputs d..d+p-1) and its
    // matrix equals gfc::Shape<d, p> (bs_encode_matches), so launch_rs_encode may take the
    // bit-sliced kernel of that shape.
    uint32_t std_encode;
};

// SHA-256 of n_parts * n_chunks chunks.  Strided mode: chunk (k, first_chunk + c) at
// base + k*part_stride + (first_chunk + c)*chunk_stride, len bytes, digest at (k*n_chunks+c)*32.
// List mode (ptrs != nullptr): item i hashes lens[i] bytes at ptrs[i] (n_parts = items,
// n_chunks = 1).
struct ShaParams {
    const uint8_t* base;
    uint64_t part_stride;
    uint64_t chunk_stride;
    uint64_t len;
    const uint64_t* ptrs;
    const uint64_t* lens;
    uint32_t n_parts;
    uint32_t first_chunk;
    uint32_t n_chunks;
    uint8_t* digests;     // may be null when only verifying
    // Verify mode (DataVerifier::verify): items with present[item] == 0 are skipped (ok = 0);
    // ok[item] = digest == expected[item*32 .. +32].  All three optional (device pointers).
    const uint8_t* present;
    const uint8_t* expected;
    uint8_t* ok;
    // Compacted item list (nullable, lane kernel only): lane g hashes item items[g] of the
    // strided batch, g < n_items; present is ignored and unlisted items are not touched.  Packs
    // the loaded chunks of a read into full waves (RS(10,4), d of 14 loaded: 640 waves, not 896).
    const uint32_t* items;
    uint32_t n_items;
};

struct FillParams {
    uint8_t* base;
    uint64_t part_stride;
    uint64_t chunk_stride;
    uint64_t len;
    uint64_t seed;
    uint32_t n_parts;
    uint32_t n_chunks;
};

// Fused encode_sep + SHA-256 of all d+p chunks (fused_kernels.hip).  Encode tables come from
// the codec's encode pattern record `pat`; digests as in ShaParams ((k*(d+p) + i) * 32).
struct FusedParams {
    uint8_t* base;
    uint64_t part_stride;
    uint64_t chunk_stride;
    uint64_t len;
    const uint32_t* pat;
    uint8_t* digests;
    uint32_t n_parts;
    uint32_t d;
    uint32_t p;
    uint32_t parts_per_wg;  // set by launch_encode_hash
    uint32_t enc_prio;      // set by launch_encode_hash: 1 = encoder waves at s_setprio 1 (2: never set)
};

hipError_t launch_rs_apply(const ApplyParams& a, bool vec16, hipStream_t s);
// encode_sep over a batch: the bit-sliced kernel of the shape when a.std_encode, the layout is
// 16-byte aligned and (d, p) is one of the compiled shapes; launch_rs_apply otherwise.
hipError_t launch_rs_encode(const ApplyParams& a, bool vec16, hipStream_t s);
// Whether a codec's parity rows (p x d bytes, row-major) are those of a compiled bit-sliced
// shape (the compile-time construction of gf_const.hpp, compared byte for byte).
bool bs_encode_matches(uint32_t d, uint32_t p, const uint8_t* parity_rows);
// Listed parts whose patterns carry their own row count (1..max_var_rows()), one launch.
// a.n_rows selects the kernel's row class (2, 4 or 8 rows) and MUST be at least the widest
// listed pattern's row count, or 0 (unknown: the 8-row class); a pattern wider than its class is
// skipped in the kernel (its chunks are not written).  The caller (capi.cpp reconstruct_batch)
// checks this against the host records before every launch.
hipError_t launch_rs_apply_var(const ApplyParams& a, bool vec16, hipStream_t s);
uint32_t max_var_rows();

// encode_sep over a ragged batch: part k's chunk i (d data then p parity) at
// base + off[k] + i * stride(L_k), stride(L) = L rounded up to 16, base and off[k] multiples of
// 16.  One wave per work unit (ragged_unit_bytes() of one part's columns); `units` is the prefix
// array over the parts' unit counts (units[0] = 0, units[n_parts] = total_units) and `parts`
// holds {off lo, off hi, L lo, L hi} per part (device memory, read as wave-uniform words).
// Exactly L_k bytes of each parity chunk are written.
// Split layout (split != 0, encode only): `parts` holds six words per part, {off, L, disp}: the
// d data chunks at base + off[k] + j * stride(L_k) as above, and output row r's chunk (index d + r
// of the record) at that address plus disp[k], a 64-bit displacement that wraps (the parity
// region may lie below the data region).  Not one byte of the data chunks is written.
// Reconstruct: the listed parts are a compact selection of the batch (those that need a rebuild),
// `parts` / `units` describe the listed parts only, and listed part lp uses the pattern record at
// pat + part_pat[lp] (word offsets into one uploaded block of records).
struct RaggedParams {
    uint8_t* base;
    const uint32_t* pat;    // the codec's encode record, or the block of decode records
    const uint32_t* units;  // [n_parts + 1]
    const uint32_t* parts;  // [n_parts][4], split: [n_parts][6]
    const uint32_t* part_pat;  // [n_parts] or null: every part uses the record at pat
    uint32_t n_parts;
    uint32_t total_units;
    uint32_t d;
    uint32_t n_rows;
    uint32_t split;  // nonzero: the split layout's records (launch_rs_encode_ragged only)
};
// Every listed part through all a.n_rows rows of its record (part_pat: records that share that
// row count), in row groups of up to max_var_rows(): the encode, and reconstruct patterns wider
// than max_var_rows().
hipError_t launch_rs_encode_ragged(const RaggedParams& a, hipStream_t s);
// Reconstruct of listed parts whose records carry their own row count (1..max_var_rows()), one
// launch.  a.part_pat is required; a.n_rows selects the row class (2, 4 or 8) and MUST be at
// least the widest listed record's row count, or 0 (the 8-row class): a wider record's part is
// skipped in the kernel.  The caller (ragged.cpp reconstruct_ragged) checks the host records first.
hipError_t launch_rs_reconstruct_ragged(const RaggedParams& a, hipStream_t s);
uint64_t ragged_unit_bytes();
uint64_t ragged_max_units();  // most units one launch can address (grid and index limits)

// The decode plan of a ragged read, built on the device from the verification's flags
// (plan_kernels.hip): one wave per part, everything device memory.  For part k of d + p chunks:
//   verified[k][i] = 1 if present[k][i] == CEC_PRESENT_VERIFIED, ok[k][i] if it is otherwise
//                    nonzero (the chunk was hashed), 0 if it is absent;
//   part_status[k] = CEC_OK with at least d verified chunks, else CEC_TOO_FEW_SHARDS_PRESENT;
//   records + k * slot_words = the part's pattern record (gf256.hpp), the one
//                    cec_codec::decode_record builds for its verified set: inputs the first d
//                    verified chunks, outputs the unverified data chunks, then (data_only == 0)
//                    the unverified parity chunks.  Word 0 = 0, and nothing behind it written,
//                    for a part that cannot be decoded or has nothing to rebuild.
// matrix: the codec's (d+p) x d coding matrix, row-major bytes.  max_rows: the most rows a part
// can need (p, or min(p, d) under data_only); slot_words >= pattern_words(d, max_rows).
struct PlanParams {
    const uint8_t* present;   // [n_parts][d+p]
    const uint8_t* ok;        // [n_parts][d+p]
    const uint8_t* matrix;
    uint8_t* verified;        // [n_parts][d+p]
    int32_t* part_status;     // [n_parts]
    uint32_t* records;        // [n_parts][slot_words]
    uint32_t n_parts;
    uint32_t d;
    uint32_t p;
    uint32_t slot_words;
    uint32_t max_rows;
    uint32_t data_only;
};
// d <= 32 (a lane per column of [A | I]) and p <= 8 (max_var_rows(), the shared reconstruct
// launch): every compiled shape.
bool decode_plan_covers(uint32_t d, uint32_t p);
hipError_t launch_decode_plan(const PlanParams& a, hipStream_t s);

// The packed return of a ragged read (plan_kernels.hip), queued behind the rebuild: everything
// the rebuild wrote, gathered into `rebuilt` in part order.  records / slot_words / max_rows: the
// planner's (PlanParams); units / parts / total_units: the whole batch's (RaggedParams), unit_bytes
// = ragged_unit_bytes(); t = d + p.
//   ret_off[k] = the sum over the parts before k of n_out * stride(L) bytes (return_plan.hpp),
//                ret_off[n_parts] = the total;
//   row r of part k (its chunk records[k][1 + d + r]) = L_k bytes at
//                rebuilt + ret_off[k] + r * stride(L_k).
// Bytes between L and the stride are unspecified; nothing at or behind ret_off[n_parts] is
// written, and that is at most the sum of max_rows * stride(L_k), which the caller's region holds.
struct ReturnParams {
    const uint8_t* base;
    const uint32_t* records;  // [n_parts][slot_words]
    const uint32_t* units;    // [n_parts + 1]
    const uint32_t* parts;    // [n_parts][4]
    uint64_t* ret_off;        // [n_parts + 1]
    uint8_t* rebuilt;
    uint64_t unit_bytes;
    uint32_t n_parts;
    uint32_t total_units;
    uint32_t d;
    uint32_t t;
    uint32_t slot_words;
    uint32_t max_rows;
};
hipError_t launch_return_plan(const ReturnParams& a, hipStream_t s);
bool fused_supported(uint32_t d, uint32_t p);
bool fused_covers(uint32_t d, uint32_t p, uint64_t len);
hipError_t launch_encode_hash(const FusedParams& a, bool vec16, hipStream_t s);

// Fused encode_sep + SHA-256 over a ragged batch in one launch (fused_kernels.hip): the layout
// and the part records of RaggedParams ({off, L} per part, split: {off, L, disp}; every output
// row's chunk at its address plus disp[k], not one byte of the data chunks written), exactly L_k
// bytes of each parity chunk written, digests at (k * (d + p) + i) * 32 of the caller's order.
// `order` lists the parts by chunk length, longest first: workgroup w takes parts
// order[w * G ..], G = parts_per_wg, and runs as many steps as its first part needs.
// Chunk lengths below 2^39 (the step count is 32-bit).
struct FusedRaggedParams {
    uint8_t* base;          // split: only read
    const uint32_t* pat;    // the codec's encode record
    const uint32_t* order;  // [n_parts]
    const uint32_t* parts;  // [n_parts][4], split: [n_parts][6]
    uint8_t* digests;
    uint32_t n_parts;
    uint32_t d;
    uint32_t p;
    uint32_t split;
    uint32_t parts_per_wg;  // set by launch_encode_hash_ragged
};
// d <= 16 and p <= 8 (the generic fused build's scope); other shapes take the two-pass path.
bool fused_ragged_covers(uint32_t d, uint32_t p);
hipError_t launch_encode_hash_ragged(const FusedRaggedParams& a, hipStream_t s);
hipError_t launch_sha256(const ShaParams& a, bool vec16, hipStream_t s);
// Whether launch_sha256 takes the split producer/rounds kernel for `chunks` chunks (small
// launches: lower latency per chain); callers pick separate encode + SHA over the fused kernel
// when it does.
bool use_split(uint64_t chunks);
int device_cus();  // CUs of the current device
// The SHA-256 lane kernel's occupancy rule (sha256_kernels.hip launch_lane): the dynamic LDS a
// 256-thread workgroup reserves so that one wave runs per SIMD (two when the grid exceeds the
// CUs), and the largest such reservation.
size_t sha_lane_reservation(uint32_t grid_x);
size_t sha_lane_reservation_max();

// Resumable SHA-256 over a list of chunk segments (sha256_resume_kernels.hip), one lane per item:
// item i hashes lens[i] bytes at ptrs[i] (16-byte aligned) onto the chain kept in the midstate
// record midstates + record[i] * 48 (segment_words.hpp ShaMidstate).  flags[i] & 1 (FIRST): the
// chain starts here, from the initial hash value and 0 prior bytes, and the record is not read.
// flags[i] & 2 (LAST): the chain ends here, with the padding of a message of prior + lens[i]
// bytes; the digest goes to digests + i * 32 and the record is not written.  Not LAST: lens[i]
// is a multiple of 64, and the eight state words and prior + lens[i] are written to the record;
// no digest byte is touched.  An item that is FIRST and LAST touches no record (midstates may be
// null when every item is).  `order` lists the n_items items the launch hashes, longest first.
struct ShaResumeParams {
    const uint64_t* ptrs;
    const uint64_t* lens;
    const uint32_t* order;
    const uint32_t* record;
    const uint8_t* flags;
    uint8_t* midstates;
    uint8_t* digests;
    uint32_t n_items;
};
hipError_t launch_sha256_resume(const ShaResumeParams& a, hipStream_t s);
// The same list with a verdict where a chain ends (sha256_resume_verify_kernel): flags[i] & 2
// (LAST): the digest of the whole message is compared with the 32 bytes at expected + i * 32
// (16-byte aligned) and ok[i] = 1 on equality, else 0; nothing else is written.  Not LAST: the
// record is written as above, and not one byte of ok is touched.
struct ShaVerifyResumeParams {
    const uint64_t* ptrs;
    const uint64_t* lens;
    const uint32_t* order;
    const uint32_t* record;
    const uint8_t* flags;
    uint8_t* midstates;
    const uint8_t* expected;
    uint8_t* ok;
    uint32_t n_items;
};
hipError_t launch_sha256_resume_verify(const ShaVerifyResumeParams& a, hipStream_t s);
hipError_t launch_fill(const FillParams& a, hipStream_t s);

// Packed <-> batch chunk moves (move_kernels.hip): packed chunk j (len bytes at packed + j*len)
// is batch chunk ids[j] = k*t + i (at batch + k*part_stride + i*chunk_stride); to_batch = 1
// scatters packed -> batch, 0 gathers batch -> packed.  Device memory on both sides.
struct MoveParams {
    uint8_t* batch;
    uint64_t part_stride;
    uint64_t chunk_stride;
    uint32_t t;
    uint8_t* packed;
    uint64_t len;
    const uint32_t* ids;
    uint32_t n;
    uint32_t to_batch;
    // nullable: chunk j of the packed side is at packed + packed_ids[j] * len (else j * len)
    const uint32_t* packed_ids = nullptr;
};
hipError_t launch_move_chunks(const MoveParams& a, hipStream_t s);

// CEC_READ_CARRY's stash, queued in the batch's own stream after the verification: every part
// with 0 < verified chunks < d (the parts wait() will report CEC_TOO_FEW_SHARDS_PRESENT) gets the
// next of the `n_reserved` pool entries the host reserved for this batch, in part order, and its
// verified chunks (present == CEC_PRESENT_VERIFIED, or loaded and ok) are copied to
// pool + (entry * t + i) * len.  map[k] = the entry of part k, or -1 (none needed, or the
// reservation ran out).
struct CarryStashParams {
    const uint8_t* batch;
    uint64_t part_stride;
    uint64_t chunk_stride;
    uint32_t t;
    uint32_t d;
    uint32_t n_parts;
    uint8_t* pool;
    uint64_t len;             // bytes per chunk copied (the pool's chunk stride)
    const uint8_t* present;   // device [n_parts][t]: the caller's loaded flags
    const uint8_t* ok;        // device [n_parts][t]: verification of the freshly loaded chunks
    const uint32_t* reserved;
    uint32_t n_reserved;
    int32_t* map;             // device [n_parts]
};
hipError_t launch_carry_stash(const CarryStashParams& a, hipStream_t s);

// Host mirror of the device generator (cec_synth_byte).
uint8_t synth_byte(uint64_t seed, uint64_t part, uint64_t chunk, uint64_t offset);

}  // namespace cec
