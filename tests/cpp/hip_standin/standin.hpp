// Test-side controls of the host HIP stand-in (standin.cpp): schedules, holds, fault injection,
// the violation / hazard lists, the operation log and the tables of live objects.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

// Everything back to the initial state (device count, seed, counters, lists, log).  Nothing may be
// live; memory of freed allocations (kept so that a late use is caught, not a crash) is returned.
void standin_reset();
void standin_set_devices(int n);
// Per queued operation a delay picked from (seed, stream, position): 0 for three in four, else up
// to 300 us.  Seed 0: no delays.
void standin_set_seed(uint64_t seed);

// A held stream runs nothing queued on it until it is released.
void standin_hold(hipStream_t s);
void standin_release(hipStream_t s);
void standin_hold_all();     // every live stream
void standin_release_all();
// Live streams in creation order.
std::vector<hipStream_t> standin_streams();
// Host functions (the compute stand-ins' launches) the stream has run.
uint64_t standin_stream_launches(hipStream_t s);

// An operation on `s` that runs fn when the queue reaches it (a kernel launch's stand-in).  `uses`
// are device pointers the launch names: each must lie in a live device allocation, which counts
// as in use until the function has run.
hipError_t standin_enqueue(hipStream_t s, const char* label, std::function<void()> fn,
                           const std::vector<const void*>& uses);
// Records a violation unless [p, p + n) lies inside one live device allocation.
void standin_check_device_range(const void* p, size_t n, const char* what);

// Fault injection: the nth (1-based) call of `name` from now returns hipErrorOutOfMemory, once.
// Names: hipMalloc, hipHostMalloc, hipStreamCreateWithFlags, hipStreamCreateWithPriority,
// hipEventCreateWithFlags.  standin_calls: calls of `name` since the last standin_reset /
// standin_clear_calls.
void standin_fail(const char* name, uint64_t nth);
uint64_t standin_calls(const char* name);
void standin_clear_calls();
extern const char* const standin_creating_calls[5];

// Mutants (the test program proves with them that it notices a missing wait).
enum StandinMutant { kMutantNone = 0, kMutantEventSyncNoWait = 1, kMutantDropStreamWaitEvent = 2 };
void standin_set_mutant(StandinMutant m);

// What the runtime never reports.  violations: misuse (dead or unknown handles, double frees,
// copies out of bounds or of the wrong kind, width > pitch, a foreign device current).  hazards:
// a free or stream destroy while queued work still names the range or stream (the real calls
// happen to synchronise).
std::vector<std::string> standin_violations();
std::vector<std::string> standin_hazards();
struct StandinLive {
    size_t device_allocs, pinned_allocs, streams, events;
    size_t total() const { return device_allocs + pinned_allocs + streams + events; }
};
StandinLive standin_live();

// The log of queued operations, in the order of the calls (off by default).
struct StandinOp {
    enum Type { Copy, Memset, Launch, EventRecord, WaitEvent } type;
    hipMemcpyKind kind;
    unsigned stream;       // creation number of the stream
    uint64_t pos;          // position in the stream's queue (1-based)
    // copies: allocation number (-1: pageable) and offset from its base for each side
    int dst_alloc, src_alloc;
    size_t dst_off, src_off;
    size_t width, rows, dpitch, spitch;
    const char* label;     // launches
};
void standin_log(bool on);
std::vector<StandinOp> standin_ops();
// Allocation number of a pointer (-1: none).
int standin_alloc_of(const void* p);
unsigned standin_stream_number(hipStream_t s);
