/* chunky_ec_scrub.h - the segmented scrub of the chunky_ec C-ABI: resumable SHA-256 verification
 * over segments of stored copies (cec_verify_segments) and the host-staged pipeline on top of it
 * (cec_scrub_pipeline_*).
 *
 * Part of the same library and the same ABI as chunky_ec.h, which includes this file: including
 * either gives both.  It is a file of its own for the reason chunky_ec_segments.h is:
 * tests/test_segments_header.py pins the functions of that header; this header and the crate's
 * `sys::scrub` block are held together by the same rules in tests/test_scrub_header.py.
 *
 * Why segments: a verification batch costs the SHA-256 chain of its longest copy, a serial lane
 * (cec_verify_ragged, cec_parts_verify).  The state of a chain after any whole number of 64-byte
 * blocks (the midstate record of chunky_ec_segments.h) can be kept and the chain resumed later, and
 * nothing depends on a copy's verdict before its last byte.  So a long copy can pass through as
 * segments of bounded length, one per call, and a call's chain is at most one segment long. */
#ifndef CHUNKY_EC_SCRUB_H
#define CHUNKY_EC_SCRUB_H

#include "chunky_ec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cec_verify_ragged(total_shards = 1) over segments of copies, device resident, queued on `stream`
 * with no wait in the call.  Entry k is seg_lens[k] bytes at base + offsets[k]: the layout of
 * cec_ragged_layout with total_shards = 1 over seg_lens, under cec_verify_ragged's alignment, order
 * and overlap rules.  Each entry continues the SHA-256 chain of its copy; flags[k] has the meanings
 * of cec_encode_hash_segments:
 *   CEC_SEG_FIRST      the chain starts with this entry; otherwise it resumes from the midstate
 *                      record the copy's previous segment left.
 *   CEC_SEG_LAST       the chain ends with this entry (of any nonzero length): the digest of the
 *                      whole copy is compared with the 32 bytes at expected + k * 32 and ok[k] is
 *                      written, 1 on equality, else 0.  Otherwise the entry's length is a multiple
 *                      of 64, the midstate is written back, row k of expected is not read and not
 *                      one byte of ok is touched.
 * State slot s owns the one record at midstates + s * cec_sha_midstate_bytes() (DEVICE memory,
 * 16-byte aligned, n_state_slots records); entry k uses slot state_slots[k].  An entry that is
 * FIRST | LAST touches no record, its slot is ignored, and its flag is what cec_verify_ragged gives
 * for that copy.  After an entry's LAST its slot's record is unspecified and the slot may serve
 * another copy.  The call keeps no state of its own: successive segments of a copy must be queued
 * in order on one stream, or ordered by the caller.  No digest is stored and `base` is never
 * written.  expected is DEVICE memory [n_segs][32], 16-byte aligned; ok is DEVICE memory [n_segs].
 * offsets, seg_lens, state_slots and flags are HOST memory, copied before the call returns.
 * Errors, all before any device use, in this order: a null pointer (midstates may be null only if
 * every entry is FIRST | LAST), and n_segs beyond the 32-bit item index, which is looked at before
 * the arrays are walked -> CEC_ERR_INVALID_ARGUMENT; a zero seg_lens[k] -> CEC_EMPTY_SHARD;
 * cec_verify_ragged's alignment, order and overlap rules; an entry without CEC_SEG_LAST whose
 * length is no multiple of 64; a slot >= n_state_slots; a slot named by two record-touching
 * entries of one call -> CEC_ERR_INVALID_ARGUMENT; then CEC_ERR_NO_DEVICE.
 * n_segs == 0 -> CEC_OK with nothing launched. */
int cec_verify_segments(const uint8_t* base, const size_t* offsets, const size_t* seg_lens,
                        size_t n_segs, const uint32_t* state_slots, const uint8_t* flags,
                        uint8_t* midstates, size_t n_state_slots, const uint8_t* expected,
                        uint8_t* ok, void* stream);

/* Host-staged scrub pipeline: cec_parts_verify with slots in flight, whose batches carry segments
 * of copies, with the midstates of the copies that are under way ("open") kept in device memory
 * between batches.  It runs on the device that is current at new; there is no codec.  One thread
 * drives a pipeline.
 * new: `depth` (1..16) slots, each with page-locked and device staging for slot_bytes of segments
 *   and the expected rows, flags and launch words of max_entries entries, one stream and one
 *   event, and one device pool of max_open midstate records, all made here and never later.
 *   max_open == 0 is legal: only whole copies.
 * acquire / query / drain / depth / free: as cec_segment_pipeline (acquire gives no data region:
 *   the engine packs).
 * submit_from: entry k is the bytes [seg_offsets[k], seg_offsets[k] + seg_lens[k]) of the copy
 *   bufs[k] of lens[k] bytes.  The engine packs the pieces 16-byte aligned into the slot, then
 *   queues one upload (pieces, expected rows, words), cec_verify_segments' launch and the copy
 *   back of the n flags.  seg_offsets[k] == 0 is FIRST; a range that ends at lens[k] is LAST.
 *   expected is HOST memory [n][32], rows read for LAST entries only.  An entry that is not both
 *   names the copy's id, open_ids[k] < max_open, which it holds from its FIRST to its LAST; the
 *   engine keeps each id's open flag and bytes so far.  An id is free again after its LAST and may
 *   be given to another copy in the next batch.
 *   Every batch's launch is ordered behind the previous batch's, whatever their slots; the copies
 *   of different slots stay unordered.
 * wait: *ok = the slot's pinned flags [n], valid for the batch's LAST entries only; *n = the
 *   batch's entries.  Valid until the slot is acquired again.
 * open_count: the ids that are open.  abandon: closes an open id after a caller's error (its copy
 *   will not be finished); CEC_ERR_INVALID_ARGUMENT if the id is not open.
 * Errors of new, before any device use: a null `out`, depth outside 1..16, max_entries == 0 or
 * beyond the 32-bit item index, slot_bytes < 16, sizes that overflow, max_open records beyond 32
 * bits -> CEC_ERR_INVALID_ARGUMENT; then CEC_ERR_NO_DEVICE.  Errors of submit_from, before any
 * device use, the slot staying usable and no id changing: a null pipeline or array, a slot out of
 * range, n > max_entries -> CEC_ERR_INVALID_ARGUMENT; a zero lens[k] or seg_lens[k] ->
 * CEC_EMPTY_SHARD; a null bufs[k]; then, each -> CEC_ERR_INVALID_ARGUMENT, the rules of
 * cec_segment_pipeline_submit_from with L_k = lens[k]: an id >= max_open; an id twice in one
 * batch; a FIRST that is not also LAST on an open id; a continuation on an id that is not open; a
 * continuation whose seg_offsets[k] is not the bytes already submitted (or whose lens[k]
 * changed); a range past lens[k]; a length without LAST that is no multiple of 64; then the slot's
 * capacity.  Error text: cec_last_error(). */
typedef struct cec_scrub_pipeline cec_scrub_pipeline;
int cec_scrub_pipeline_new(size_t slot_bytes, size_t max_entries, size_t depth, size_t max_open,
                           cec_scrub_pipeline** out);
void cec_scrub_pipeline_free(cec_scrub_pipeline* pipeline);
size_t cec_scrub_pipeline_depth(const cec_scrub_pipeline* pipeline);
int cec_scrub_pipeline_acquire(cec_scrub_pipeline* pipeline, size_t* slot);
int cec_scrub_pipeline_submit_from(cec_scrub_pipeline* pipeline, size_t slot,
                                   const uint8_t* const* bufs, const size_t* lens,
                                   const size_t* seg_offsets, const size_t* seg_lens,
                                   const uint32_t* open_ids, const uint8_t* expected, size_t n);
int cec_scrub_pipeline_wait(cec_scrub_pipeline* pipeline, size_t slot, const uint8_t** ok,
                            size_t* n);
int cec_scrub_pipeline_query(cec_scrub_pipeline* pipeline, size_t slot);
int cec_scrub_pipeline_drain(cec_scrub_pipeline* pipeline);
size_t cec_scrub_pipeline_open_count(const cec_scrub_pipeline* pipeline);
int cec_scrub_pipeline_abandon(cec_scrub_pipeline* pipeline, uint32_t id);

#ifdef __cplusplus
}
#endif

#endif /* CHUNKY_EC_SCRUB_H */
