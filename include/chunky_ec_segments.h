/* chunky_ec_segments.h - segmented ragged writes of the chunky_ec C-ABI: resumable SHA-256 over
 * column segments of parts (cec_encode_hash_segments) and the host-staged pipeline on top of it
 * (cec_segment_pipeline_*).
 *
 * Part of the same library and the same ABI as chunky_ec.h, which includes this file: including
 * either gives both.  It is a file of its own for the reason chunky_ec_parts_read.h is:
 * tests/test_parts_header.py pins the functions of chunky_ec_parts.h; this header and the crate's
 * `sys::segments` block are held together by the same rules in tests/test_segments_header.py.
 *
 * Why segments: a ragged batch costs the SHA-256 chain of its longest chunk, a serial lane.
 * Reed-Solomon is independent per byte column, and SHA-256's state after any whole number of
 * 64-byte blocks (the midstate) can be kept and the chain resumed later.  So a part with long
 * chunks can pass through as column segments of bounded length, one per call, and a call's chain
 * is at most one segment long. */
#ifndef CHUNKY_EC_SEGMENTS_H
#define CHUNKY_EC_SEGMENTS_H

#include "chunky_ec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Entry flags: the entry holds the first / the last columns of its part's chunks.  A whole part is
 * CEC_SEG_FIRST | CEC_SEG_LAST. */
#define CEC_SEG_FIRST 1u
#define CEC_SEG_LAST 2u

/* Bytes of one midstate record: 48 (eight 32-bit state words, the 64-bit count of bytes hashed so
 * far, 8 reserved bytes).  Records are 16-byte aligned; their content is the engine's own. */
size_t cec_sha_midstate_bytes(void);

/* cec_encode_hash_split over column segments, device resident.  Entry k is the columns
 * [a, a + seg_lens[k]) of one part, laid out as an entry of cec_split_layout over seg_lens: data
 * piece j (j < d) is seg_lens[k] bytes at data_base + data_offsets[k] + j *
 * cec_ragged_stride(seg_lens[k]), and parity piece i likewise under parity_base.  Queued on
 * `stream`: the parity pieces of every entry (exactly seg_lens[k] bytes of each are written; the
 * parity of a column range is the parity of that range alone), then SHA-256 of all d + p pieces,
 * each continuing the chain of its chunk:
 *   CEC_SEG_FIRST      the chain starts with this piece; otherwise it resumes from the midstate
 *                      record the previous segment left.
 *   CEC_SEG_LAST       the chain ends with this piece (of any nonzero length): the digest of the
 *                      whole chunk is written to digests + (k * (d + p) + i) * 32.  Otherwise the
 *                      piece's length is a multiple of 64, the midstate is written back, and not
 *                      one byte of the entry's digest rows is touched.
 * State slot s owns the d + p records at midstates + (s * (d + p) + i) * 48 (DEVICE memory,
 * 16-byte aligned, n_state_slots * (d + p) records); entry k uses slot state_slots[k].  An entry
 * that is FIRST | LAST touches no record, its slot is ignored, and it gives what
 * cec_encode_hash_split gives for that part.  After an entry's LAST its slot's records are
 * unspecified and the slot may serve another part.  The call keeps no state of its own:
 * successive segments of a chunk must be queued in order on one stream, or ordered by the caller.
 * All arrays but data, parity, midstates and digests are HOST memory, copied before the call
 * returns.
 * Errors, all before any device use, in this order: a null pointer (midstates may be null only if
 * every entry is FIRST | LAST) -> CEC_ERR_INVALID_ARGUMENT; a zero seg_lens[k] ->
 * CEC_EMPTY_SHARD; cec_encode_hash_split's alignment, order and overlap rules; an entry without
 * CEC_SEG_LAST whose length is no multiple of 64; a slot >= n_state_slots; a slot named by two
 * record-touching entries of one call -> CEC_ERR_INVALID_ARGUMENT; then CEC_ERR_NO_DEVICE.
 * n_segs == 0 -> CEC_OK with nothing launched. */
int cec_encode_hash_segments(const cec_codec* codec, const uint8_t* data_base,
                             const size_t* data_offsets, uint8_t* parity_base,
                             const size_t* parity_offsets, const size_t* seg_lens, size_t n_segs,
                             const uint32_t* state_slots, const uint8_t* flags, uint8_t* midstates,
                             size_t n_state_slots, uint8_t* digests, void* stream);

/* Host-staged segment pipeline: cec_parts_pipeline whose batches carry column segments, with the
 * midstates of the parts that are under way ("open") kept in device memory between batches.
 * new: as cec_parts_pipeline_new, plus a device pool of max_open * (d + p) midstate records.
 *   max_open == 0 is legal: only whole parts.
 * acquire / query / drain / depth / free: as the parts pipeline (acquire gives no data region:
 *   the engine packs).
 * submit_from: part k is lengths[k] bytes at data_bufs[k], L_k = ceil(lengths[k] / d) (returned in
 *   chunksizes[k]).  The batch carries columns [seg_offsets[k], seg_offsets[k] + seg_lens[k]) of
 *   each of its d chunks: the engine packs piece j from the part's bytes
 *   [j * L_k + seg_offsets[k], + seg_lens[k]), clipped to lengths[k], zeros behind, then queues
 *   one upload, cec_encode_hash_segments and the copies back of the parity pieces and the digests.
 *   seg_offsets[k] == 0 is FIRST; a range that ends at L_k is LAST.  An entry that is not both
 *   names the part's id, open_ids[k] < max_open, which it holds from its FIRST to its LAST; the
 *   engine keeps each id's open flag and columns so far.  An id is free again after its LAST and
 *   may be given to another part in the next batch.
 *   Every batch's SHA-256 launch is ordered behind the previous batch's, whatever their slots;
 *   the copies of different slots stay unordered.
 * wait: *parity = the slot's pinned parity region, the parity pieces in the cec_split_layout of
 *   the batch's seg_lens; *digests = [n][d+p][32], rows valid for LAST entries only; *n = the
 *   batch's entries.  Valid until the slot is acquired again.
 * open_count: the ids that are open.  abandon: closes an open id after a caller's error (its part
 *   will not be finished); CEC_ERR_INVALID_ARGUMENT if the id is not open.
 * Errors of new: those of cec_parts_pipeline_new, and a max_open whose pool overflows.  Errors of
 * submit_from, before any device use, the slot staying usable and no id changing: those of
 * cec_parts_pipeline_submit_from (null arrays among them; a zero seg_lens[k] -> CEC_EMPTY_SHARD),
 * then, each -> CEC_ERR_INVALID_ARGUMENT: an id >= max_open; an id twice in one batch; a FIRST
 * that is not also LAST on an open id; a continuation on an id that is not open; a continuation
 * whose seg_offsets[k] is not the columns already submitted (or whose lengths[k] changed); a range
 * past L_k; a length without LAST that is no multiple of 64; then the slot's capacity.  Error
 * text: cec_last_error(). */
typedef struct cec_segment_pipeline cec_segment_pipeline;
int cec_segment_pipeline_new(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts,
                             size_t depth, size_t max_open, cec_segment_pipeline** out);
void cec_segment_pipeline_free(cec_segment_pipeline* pipeline);
size_t cec_segment_pipeline_depth(const cec_segment_pipeline* pipeline);
int cec_segment_pipeline_acquire(cec_segment_pipeline* pipeline, size_t* slot);
int cec_segment_pipeline_submit_from(cec_segment_pipeline* pipeline, size_t slot,
                                     const uint8_t* const* data_bufs, const size_t* lengths,
                                     const size_t* seg_offsets, const size_t* seg_lens,
                                     const uint32_t* open_ids, size_t n_parts, size_t* chunksizes);
int cec_segment_pipeline_wait(cec_segment_pipeline* pipeline, size_t slot, const uint8_t** parity,
                              const uint8_t** digests, size_t* n_parts);
int cec_segment_pipeline_query(cec_segment_pipeline* pipeline, size_t slot);
int cec_segment_pipeline_drain(cec_segment_pipeline* pipeline);
size_t cec_segment_pipeline_open_count(const cec_segment_pipeline* pipeline);
int cec_segment_pipeline_abandon(cec_segment_pipeline* pipeline, uint32_t id);

#ifdef __cplusplus
}
#endif

#endif /* CHUNKY_EC_SEGMENTS_H */
