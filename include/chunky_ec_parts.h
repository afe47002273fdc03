/* chunky_ec_parts.h - the ragged write pipeline of the chunky_ec C-ABI (cec_parts_pipeline_*).
 *
 * Part of the same library and the same ABI as chunky_ec.h, which includes this file: including
 * either gives both.  It is a file of its own because the check that holds chunky_ec.h and the
 * Rust crate's main extern block together (tests/test_rust_conformance.py) knows a fixed list of
 * handle types; this header and the crate's `sys::parts` block are held together by the same
 * rules in tests/test_parts_header.py. */
#ifndef CHUNKY_EC_PARTS_H
#define CHUNKY_EC_PARTS_H

#include "chunky_ec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-staged ragged write pipeline: cec_parts_encode with slots in flight, for parts whose chunk
 * lengths differ (whole small files, short last parts).  `depth` (1..16) slots on the current
 * device; one thread drives a pipeline.  A slot owns a pinned data region of slot_data_bytes, a
 * pinned parity region of slot_data_bytes / d * p (plus slack) and pinned digests for max_parts
 * parts, device regions of the same sizes, one stream and one event; everything is made by
 * cec_parts_pipeline_new (an allocation failure is reported there) and free restores the
 * caller's device.  A batch lies in the slot in the packed split layout (cec_split_layout).
 * acquire: the next slot in round-robin order; waits for the slot's previous batch, whose results
 *   are void from then on; *data = the slot's pinned data region.
 * submit: the caller has written the batch there (every data chunk its chunk_lens[k] bytes, zeros
 *   behind the file's bytes).  Queues one H2D of exactly the data bytes, the launches of
 *   cec_encode_hash_split, one D2H of exactly the parity bytes and one of the digests on the
 *   slot's stream and returns without waiting.
 * submit_from: cec_parts_encode's form.  Part k is lengths[k] bytes at data_bufs[k] (only those
 *   are read), L_k = ceil(lengths[k] / d) goes to chunksizes[k]; the engine packs and zero-pads
 *   the parts into the slot (synchronously, on host threads) and continues as submit, so the
 *   packing of one slot overlaps the copies and kernels of the others.
 * wait: *parity = the slot's pinned parity region, part k's parity chunk i at
 *   parity_offsets[k] + i * cec_ragged_stride(L_k), bytes between chunks unspecified; *digests =
 *   [n_parts][d+p][32]; *n_parts = the batch's parts (0 when the slot has none, as
 *   cec_pipeline_wait).  All valid until the slot is acquired again.
 * query: 1 when the slot's batch is complete or none is in flight, 0 while it runs; never blocks.
 * Errors of new, before any device use: a null pointer, depth == 0 or > 16, max_parts == 0,
 * slot_data_bytes < d*16 or sizes that overflow -> CEC_ERR_INVALID_ARGUMENT; then
 * CEC_ERR_NO_DEVICE.  Errors of the submits, before any device use (the slot stays usable): null
 * pointers, n_parts > max_parts -> CEC_ERR_INVALID_ARGUMENT; a zero length -> CEC_EMPTY_SHARD; a
 * batch whose padded data (sum of d * cec_ragged_stride(L_k)) exceeds slot_data_bytes ->
 * CEC_ERR_INVALID_ARGUMENT.  n_parts == 0 is a batch of nothing -> CEC_OK.  Error text:
 * cec_last_error(). */
typedef struct cec_parts_pipeline cec_parts_pipeline;
int cec_parts_pipeline_new(const cec_codec* codec, size_t slot_data_bytes, size_t max_parts,
                           size_t depth, cec_parts_pipeline** out);
void cec_parts_pipeline_free(cec_parts_pipeline* pipeline);
size_t cec_parts_pipeline_depth(const cec_parts_pipeline* pipeline);
int cec_parts_pipeline_acquire(cec_parts_pipeline* pipeline, size_t* slot, uint8_t** data);
int cec_parts_pipeline_submit(cec_parts_pipeline* pipeline, size_t slot, const size_t* chunk_lens,
                              size_t n_parts);
int cec_parts_pipeline_submit_from(cec_parts_pipeline* pipeline, size_t slot,
                                   const uint8_t* const* data_bufs, const size_t* lengths,
                                   size_t n_parts, size_t* chunksizes);
int cec_parts_pipeline_wait(cec_parts_pipeline* pipeline, size_t slot, const uint8_t** parity,
                            const uint8_t** digests, size_t* n_parts);
int cec_parts_pipeline_query(cec_parts_pipeline* pipeline, size_t slot);
int cec_parts_pipeline_drain(cec_parts_pipeline* pipeline);

#ifdef __cplusplus
}
#endif

#endif /* CHUNKY_EC_PARTS_H */
