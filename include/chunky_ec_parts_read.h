/* chunky_ec_parts_read.h - the ragged read with a packed return and the ragged read pipeline of
 * the chunky_ec C-ABI (cec_read_ragged_packed_async, cec_parts_reader_*).
 *
 * Part of the same library and the same ABI as chunky_ec.h, which includes this file: including
 * either gives both.  It is a file of its own for the reason chunky_ec_parts.h is: the check that
 * holds chunky_ec.h and the Rust crate's main extern block together knows a fixed list of handle
 * types, and tests/test_parts_header.py pins the functions of chunky_ec_parts.h; this header and
 * the crate's `sys::parts_read` block are held together by the same rules in
 * tests/test_parts_read_header.py. */
#ifndef CHUNKY_EC_PARTS_READ_H
#define CHUNKY_EC_PARTS_READ_H

#include "chunky_ec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cec_read_ragged_async (data_only != 0) / cec_resilver_ragged_async (data_only == 0) with a
 * packed return: the same arguments, the same checks in the same order, and `base` is left byte
 * for byte as that call leaves it.  Queued behind the rebuild on `stream`, the device gathers
 * every chunk the rebuild wrote into `rebuilt` (DEVICE memory, 16-byte aligned, rebuilt_cap
 * bytes), dense and in part order, and the n_parts + 1 byte offsets are copied into
 * rebuilt_offsets (HOST memory) by a copy queued on `stream`, like `verified`: all results are
 * valid once the stream has reached that point.
 * In a part with part_status CEC_OK the slots i (ascending) with !verified[k][i] && (i < d ||
 * !data_only) are the rebuilt ones; the r-th of them is L_k bytes at
 * rebuilt + rebuilt_offsets[k] + r * cec_ragged_stride(L_k).  Other parts return nothing
 * (rebuilt_offsets[k + 1] == rebuilt_offsets[k]); rebuilt_offsets[n_parts] is the total.  Bytes
 * between L_k and the stride are unspecified; not one byte at or behind the total is written.
 * Errors, all before anything is queued, behind those of cec_read_ragged_async: a null `rebuilt`
 * or `rebuilt_offsets` (with the other null pointers), then a `rebuilt` that is not 16-byte
 * aligned, a shape outside the device planner (d > 32 or p > 8: use the calls without a packed
 * return), a rebuilt_cap below the batch's worst case, the sum of rows * cec_ragged_stride(L_k)
 * with rows = p, or min(p, d) under data_only -> CEC_ERR_INVALID_ARGUMENT, the reason in
 * cec_last_error().  n_parts == 0 -> CEC_OK, and rebuilt_offsets[0] = 0 if that pointer is set. */
int cec_read_ragged_packed_async(const cec_codec* codec, uint8_t* base, const size_t* part_offsets,
                                 const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                                 const uint8_t* expected, int data_only, uint8_t* verified,
                                 int* part_status, uint8_t* rebuilt, size_t rebuilt_cap,
                                 size_t* rebuilt_offsets, void* stream);

/* Host-staged ragged read pipeline: cec_parts_read with slots in flight and only the rebuilt
 * chunks coming back.  `depth` (1..16) slots on the current device; one thread drives a reader.
 * A slot owns a pinned staging region of slot_bytes and a device region of the same size (a batch
 * lies in both in the cec_ragged_layout(d + p, ...) layout), a device and a pinned return region
 * of slot_bytes / (d + p) * rows + rows * 16 bytes (rows = p, or min(p, d) under data_only),
 * pinned and device room for max_parts parts' digests, flags, statuses and offsets, one stream and
 * one event; everything is made by cec_parts_reader_new and free restores the caller's device.
 * acquire: the next slot in round-robin order; waits for the slot's previous batch, whose results
 *   are void from then on; *stage = the slot's pinned staging region.
 * submit: the caller has written every loaded chunk (present[k][i] != 0) there, chunk i of part k
 *   at part_offsets[k] + i * cec_ragged_stride(L_k) of cec_ragged_layout.  Queues on the slot's
 *   stream the upload of `expected` and of the loaded chunks, cec_read_ragged_packed_async into
 *   the slot's return region, the copies of the flags, statuses and offsets, and the copy of the
 *   first `guess` bytes of the return region, and returns without waiting.  guess = what the
 *   host knows will be rebuilt: over the parts with at least d chunks loaded, cec_ragged_stride(L_k)
 *   times the slots of the mode that are not loaded.  present and expected are copied before
 *   the call returns.
 * submit_from: cec_parts_read's form.  shards[k * (d + p) + i] = the caller's L_k bytes of that
 *   slot; the engine packs the loaded ones into the staging (synchronously, on host threads) and
 *   continues as submit.  The same NULL rule as cec_parts_read: a loaded slot, and in a part with
 *   at least d loaded chunks every slot the mode fills, must not be NULL.
 * wait: waits for the slot's batch.  If more was rebuilt than guessed (a loaded chunk failed its
 *   verification), the rest of the return region is fetched by one more copy (a tail copy).
 *   *verified = [n_parts][d+p], *part_status = [n_parts], *rebuilt = the pinned return region and
 *   *rebuilt_offsets = [n_parts + 1] as cec_read_ragged_packed_async gives them, *n_parts = the
 *   batch's parts (0 when the slot has none).  All valid until the slot is acquired again.
 * scatter: after wait, copies every rebuilt chunk into the caller's slot of the same array form
 *   as submit_from (exactly the slots cec_parts_read writes; nothing else is touched).  The NULL
 *   rule is checked before the first byte is copied.
 * query: 1 when the slot's batch is complete or none is in flight, 0 while it runs; never blocks.
 * stats: bytes queued to the device (digests and loaded chunks) and bytes copied back from the
 *   return region since new, and the tail copies among them.
 * Errors of new, before any device use: a null pointer, depth == 0 or > 16, max_parts == 0,
 * slot_bytes < (d+p)*16, sizes that overflow, a shape outside the device planner (d > 32 or
 * p > 8) -> CEC_ERR_INVALID_ARGUMENT; then CEC_ERR_NO_DEVICE.  Errors of the submits, before any
 * device use (the slot stays usable): a null reader, a slot out of range, null arrays with
 * n_parts != 0, n_parts > max_parts -> CEC_ERR_INVALID_ARGUMENT; a zero length ->
 * CEC_EMPTY_SHARD; the NULL rule (submit_from) and a batch whose layout (the sum of
 * (d+p) * cec_ragged_stride(L_k)) exceeds slot_bytes -> CEC_ERR_INVALID_ARGUMENT.  n_parts == 0 is
 * a batch of nothing -> CEC_OK.  Error text: cec_last_error(). */
typedef struct cec_parts_reader cec_parts_reader;
int cec_parts_reader_new(const cec_codec* codec, size_t slot_bytes, size_t max_parts, size_t depth,
                         int data_only, cec_parts_reader** out);
void cec_parts_reader_free(cec_parts_reader* reader);
size_t cec_parts_reader_depth(const cec_parts_reader* reader);
int cec_parts_reader_acquire(cec_parts_reader* reader, size_t* slot, uint8_t** stage);
int cec_parts_reader_submit(cec_parts_reader* reader, size_t slot, const size_t* chunk_lens,
                            size_t n_parts, const uint8_t* present, const uint8_t* expected);
int cec_parts_reader_submit_from(cec_parts_reader* reader, size_t slot,
                                 const uint8_t* const* shards, const size_t* chunk_lens,
                                 size_t n_parts, const uint8_t* present, const uint8_t* expected);
int cec_parts_reader_wait(cec_parts_reader* reader, size_t slot, const uint8_t** verified,
                          const int** part_status, const uint8_t** rebuilt,
                          const size_t** rebuilt_offsets, size_t* n_parts);
int cec_parts_reader_scatter(cec_parts_reader* reader, size_t slot, uint8_t* const* shards);
int cec_parts_reader_query(cec_parts_reader* reader, size_t slot);
int cec_parts_reader_drain(cec_parts_reader* reader);
void cec_parts_reader_stats(const cec_parts_reader* reader, uint64_t* bytes_up,
                            uint64_t* bytes_down, uint64_t* tail_copies);

#ifdef __cplusplus
}
#endif

#endif /* CHUNKY_EC_PARTS_READ_H */
