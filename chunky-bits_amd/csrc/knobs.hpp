// Environment knobs of the engine, read ONCE per process.
//
// Every knob is parsed into one immutable snapshot on first use; the launch paths read the
// snapshot, never the environment.  The knobs are capacities and diagnostics, plus the test
// knobs that force one of the library's own paths at test sizes (CEC_APPLY_BS,
// CEC_APPLY_MAX_BLOCKS, CEC_SHA_VARIANT 1/2, CEC_FUSED_MODE 3, CEC_FUSED, CEC_RAGGED_FUSED, CEC_COALESCE_MIXED).
// The reference calls the hot path from tokio worker threads (writer.rs:200-210 spawns a task
// per part; file_part.rs:161 runs the encode inside block_in_place), and getenv racing a setenv
// elsewhere in the host process is undefined behaviour; a snapshot read is a plain load.
//
// cec_reload_knobs() (include/chunky_ec.h, test-only) re-reads the environment into a fresh
// snapshot: the tests that flip a knob set the variable, reload, and reload again after
// restoring it.  Snapshots are never freed (a launch on another thread may still hold the old
// one); a reload costs one small allocation.
#pragma once

#include <cstddef>
#include <cstdint>

namespace cec {

struct Knobs {
    // rs_kernels.hip (meanings at each knob's use)
    uint64_t apply_max_blocks = 0;  // CEC_APPLY_MAX_BLOCKS (0: unset)
    bool apply_bs = true;           // CEC_APPLY_BS
    // sha256_kernels.hip / fused_kernels.hip
    int sha_variant = 0;            // CEC_SHA_VARIANT (raw value; only 1 and 2 are honoured)
    int fused_mode = 0;             // CEC_FUSED_MODE (raw value; only 3 is honoured)
    // capi.cpp (fused), percall.cpp, ragged.cpp
    int fused = -1;                 // CEC_FUSED 0/1 (-1: by batch size)
    int ragged_fused = -1;          // CEC_RAGGED_FUSED 0/1 (-1: by batch size, ragged.cpp)
    uint32_t coalesce_us = 200;     // CEC_COALESCE_US
    size_t coalesce_max_bytes = size_t(1024) << 20;  // CEC_COALESCE_MAX_MIB
    bool coalesce_trace = false;    // CEC_COALESCE_TRACE
    uint32_t coalesce_inflight = 2;      // CEC_COALESCE_INFLIGHT (1..16)
    int coalesce_mixed = -1;        // CEC_COALESCE_MIXED 0/1 (-1: percall.cpp's default)
    size_t idle_staging_bytes = size_t(1) << 30;  // CEC_IDLE_STAGING_MIB (per device)
    // multi.cpp
    unsigned multi_copy_threads = 4;     // CEC_MULTI_COPY_THREADS (1..32)
};

// The current snapshot (parsed on first call).
const Knobs& knobs();
// Parse the environment into a new snapshot and make it current.
void reload_knobs();

}  // namespace cec
