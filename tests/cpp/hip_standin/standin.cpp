// The host HIP stand-in: hip/hip_runtime.h's 26 calls on CPU threads, keeping what matters for
// ordering and lifetime (in-order streams that truly run beside the host, events that capture a
// position, blocking copies of pageable memory, per-thread devices and sticky errors), and
// checking what a GPU never reports (standin.hpp).
//
// Bookkeeping must not order project threads that HIP would not order, or ThreadSanitizer would
// miss their races.  The tables of allocations, streams and events are fixed arrays of slots whose
// fields are relaxed atomics (no lock, no release/acquire pair); handles are pointers into them,
// so a dead or foreign handle is told by address and state without touching a shared map.  The
// edges that remain: a stream's own mutex (taken by whoever queues on, waits for or holds that
// stream: queue -> run and run -> wait are HIP's own edges; two host threads that queue on the
// SAME stream are ordered one after the other, which HIP does not promise), and the mutex of the
// violation lists (taken only when something is already wrong).
#include "standin.hpp"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <sstream>
#include <thread>

// Freed allocations stay mapped until standin_reset (a late DEVICE-side use is then a recorded
// violation, not a crash); for the host they are dead: filled with 0xDD and, under
// AddressSanitizer, poisoned, so project host code that still reads a freed pinned buffer shows.
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

namespace {

constexpr auto R = std::memory_order_relaxed;
constexpr size_t kMaxAllocs = 1 << 14, kMaxStreams = 1 << 11, kMaxEvents = 1 << 15,
                 kMaxOps = 1 << 16;
constexpr size_t kAlign = 256;

thread_local int t_device = 0;
thread_local hipError_t t_error = hipSuccess;

std::atomic<int> g_devices{1};
std::atomic<uint64_t> g_seed{0};
std::atomic<int> g_mutant{0};
std::atomic<bool> g_log{false};

std::mutex g_list_mu;
std::vector<std::string> g_violations, g_hazards;

void report(std::vector<std::string>& list, const char* call, const std::string& what) {
    std::ostringstream os;
    os << call << ": " << what << " [thread " << std::this_thread::get_id() << "]";
    std::lock_guard<std::mutex> lk(g_list_mu);
    list.push_back(os.str());
}
void violation(const char* call, const std::string& what) { report(g_violations, call, what); }
void hazard(const char* call, const std::string& what) { report(g_hazards, call, what); }

hipError_t fail(hipError_t e) {
    if (e != hipSuccess && e != hipErrorNotReady) t_error = e;
    return e;
}

// ---- allocations ----
enum { kNone = 0, kDevice = 1, kPinned = 2 };
struct Alloc {
    std::atomic<uintptr_t> base{0};
    std::atomic<size_t> size{0};
    std::atomic<int> kind{kNone};
    std::atomic<int> live{0};
    std::atomic<int> device{0};
    std::atomic<int> pending{0};  // queued operations that name it
    std::atomic<void*> raw{nullptr};
};
Alloc g_allocs[kMaxAllocs];
std::atomic<size_t> g_nallocs{0};

Alloc* find_alloc(const void* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const size_t n = std::min(g_nallocs.load(R), kMaxAllocs);
    for (size_t i = 0; i < n; ++i) {
        Alloc& x = g_allocs[i];
        if (x.kind.load(R) == kNone) continue;
        const uintptr_t b = x.base.load(R);
        if (a >= b && a < b + x.size.load(R)) return &x;
    }
    return nullptr;
}
int alloc_number(const Alloc* a) { return a ? int(a - g_allocs) : -1; }

// ---- fault injection ----
std::atomic<uint64_t> g_calls[5], g_fail_at[5];
int call_index(const char* name) {
    for (int i = 0; i < 5; ++i)
        if (!std::strcmp(name, standin_creating_calls[i])) return i;
    std::fprintf(stderr, "standin: no creating call named %s\n", name);
    std::abort();
}
bool injected(int idx) {
    const uint64_t n = g_calls[idx].fetch_add(1, R) + 1;
    uint64_t want = n;
    return g_fail_at[idx].compare_exchange_strong(want, 0, R);
}

// ---- streams ----
struct Op {
    std::function<void()> fn;
    Alloc* uses[4] = {nullptr, nullptr, nullptr, nullptr};
    bool launch = false;
};

}  // namespace

struct ihipStream_t {
    std::atomic<int> state{0};  // 0 never made, 1 live, 2 destroyed
    std::atomic<unsigned> gen{0};
    std::atomic<int> device{0}, priority{0};
    std::atomic<uint64_t> enq{0}, done{0}, launches{0};
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Op> q;  // guarded by mu
    bool held = false, quit = false;
    std::thread th;
};

struct ihipEvent_t {
    std::atomic<int> state{0};
    std::atomic<int> device{0};
    // the last record: stream, its generation and the position captured (null: never recorded)
    std::atomic<ihipStream_t*> stream{nullptr};
    std::atomic<unsigned> gen{0};
    std::atomic<uint64_t> pos{0};
};

namespace {

ihipStream_t g_streams[kMaxStreams];
ihipEvent_t g_events[kMaxEvents];
std::atomic<size_t> g_nstreams{0}, g_nevents{0};

StandinOp g_ops[kMaxOps];
std::atomic<size_t> g_nops{0};

void log_op(const StandinOp& op) {
    if (!g_log.load(R)) return;
    const size_t i = g_nops.fetch_add(1, R);
    if (i < kMaxOps) g_ops[i] = op;
}

ihipStream_t* stream_ok(hipStream_t s, const char* call) {
    if (s < g_streams || s >= g_streams + kMaxStreams ||
        (reinterpret_cast<uintptr_t>(s) - reinterpret_cast<uintptr_t>(g_streams)) % sizeof(ihipStream_t)) {
        violation(call, s ? "a stream that was never created" : "the null stream");
        return nullptr;
    }
    const int st = s->state.load(R);
    if (st != 1) {
        violation(call, st == 2 ? "a destroyed stream" : "a stream that was never created");
        return nullptr;
    }
    return s;
}

ihipEvent_t* event_ok(hipEvent_t e, const char* call) {
    if (e < g_events || e >= g_events + kMaxEvents ||
        (reinterpret_cast<uintptr_t>(e) - reinterpret_cast<uintptr_t>(g_events)) % sizeof(ihipEvent_t)) {
        violation(call, "an event that was never created");
        return nullptr;
    }
    const int st = e->state.load(R);
    if (st != 1) {
        violation(call, st == 2 ? "a destroyed event" : "an event that was never created");
        return nullptr;
    }
    return e;
}

uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

void stream_main(ihipStream_t* s) {
    const unsigned number = unsigned(s - g_streams);
    std::unique_lock<std::mutex> lk(s->mu);
    for (;;) {
        s->cv.wait(lk, [&] { return s->quit || (!s->held && !s->q.empty()); });
        if (s->q.empty()) break;  // quit, and drained
        Op op = std::move(s->q.front());
        s->q.pop_front();
        const uint64_t pos = s->done.load(R) + 1;
        lk.unlock();
        const uint64_t seed = g_seed.load(R);
        if (seed) {
            const uint64_t r = mix(seed ^ (uint64_t(number) << 40) ^ pos);
            if ((r & 3) == 0) std::this_thread::sleep_for(std::chrono::microseconds((r >> 8) % 300));
        }
        op.fn();
        for (Alloc* a : op.uses)
            if (a) a->pending.fetch_sub(1, std::memory_order_release);  // read with acquire only by
                                                                        // a free that found it nonzero
        if (op.launch) s->launches.fetch_add(1, R);
        op.fn = nullptr;
        lk.lock();
        s->done.store(pos, std::memory_order_release);
        s->cv.notify_all();
    }
}

// Queue op on s; returns its position.
uint64_t enqueue(ihipStream_t* s, Op op) {
    for (Alloc* a : op.uses)
        if (a) a->pending.fetch_add(1, R);
    std::lock_guard<std::mutex> lk(s->mu);
    s->q.push_back(std::move(op));
    const uint64_t pos = s->enq.load(R) + 1;
    s->enq.store(pos, R);
    s->cv.notify_all();
    return pos;
}

void wait_pos(ihipStream_t* s, unsigned gen, uint64_t pos) {
    std::unique_lock<std::mutex> lk(s->mu);
    s->cv.wait(lk, [&] {
        return s->gen.load(R) != gen || s->state.load(R) != 1 ||
               s->done.load(std::memory_order_acquire) >= pos;
    });
}

bool reached(ihipStream_t* s, unsigned gen, uint64_t pos) {
    return s->gen.load(R) != gen || s->state.load(R) != 1 ||
           s->done.load(std::memory_order_acquire) >= pos;
}

hipError_t make_stream(hipStream_t* out, int priority, int idx) {
    if (!out) return fail(hipErrorInvalidValue);
    if (injected(idx)) return fail(hipErrorOutOfMemory);
    const size_t i = g_nstreams.fetch_add(1, R);
    if (i >= kMaxStreams) {
        std::fprintf(stderr, "standin: stream table full\n");
        std::abort();
    }
    ihipStream_t* s = &g_streams[i];
    s->device.store(t_device, R);
    s->priority.store(priority, R);
    s->enq.store(0, R);
    s->done.store(0, R);
    s->launches.store(0, R);
    s->held = false;
    s->quit = false;
    s->gen.fetch_add(1, R);
    s->state.store(1, R);
    s->th = std::thread(stream_main, s);
    *out = s;
    return hipSuccess;
}

// One side of a copy: the allocation it lies in (null: pageable host memory).  extent bytes from p
// must lie inside it; a device side must be live device memory.
struct Side {
    Alloc* a = nullptr;
    bool device = false;
    bool bad = false;  // dead or out of bounds: the operation is not run
};
Side side_of(const void* p, size_t extent, const char* call, const char* which) {
    Side s;
    s.a = find_alloc(p);
    if (!s.a) return s;
    s.device = s.a->kind.load(R) == kDevice;
    const uintptr_t b = s.a->base.load(R), x = reinterpret_cast<uintptr_t>(p);
    std::ostringstream os;
    if (!s.a->live.load(R)) {
        os << which << " lies in freed " << (s.device ? "device" : "pinned") << " allocation #"
           << alloc_number(s.a);
        violation(call, os.str());
        s.bad = true;
    } else if (x + extent > b + s.a->size.load(R)) {
        os << which << " [" << (x - b) << ", " << (x - b + extent) << ") runs past "
           << (s.device ? "device" : "pinned") << " allocation #" << alloc_number(s.a) << " of "
           << s.a->size.load(R) << " bytes";
        violation(call, os.str());
        s.bad = true;
    }
    return s;
}

hipError_t copy2d(const char* call, void* dst, size_t dpitch, const void* src, size_t spitch,
                  size_t width, size_t rows, hipMemcpyKind kind, hipStream_t stream) {
    ihipStream_t* s = stream_ok(stream, call);
    if (!s) return fail(hipErrorInvalidResourceHandle);
    if (width == 0 || rows == 0) return hipSuccess;
    if (!dst || !src) {
        violation(call, "null pointer");
        return fail(hipErrorInvalidValue);
    }
    if (width > dpitch || width > spitch) {
        violation(call, "width > pitch");
        return fail(hipErrorInvalidValue);
    }
    const Side d = side_of(dst, (rows - 1) * dpitch + width, call, "destination");
    const Side r = side_of(src, (rows - 1) * spitch + width, call, "source");
    if (d.bad || r.bad) return fail(hipErrorInvalidValue);
    const bool want_dd = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
    const bool want_sd = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
    if (kind != hipMemcpyDefault && (d.device != want_dd || r.device != want_sd))
        violation(call, "the copy kind contradicts the pointers' kinds");
    if (d.device && d.a->device.load(R) != s->device.load(R))
        violation(call, "device memory of another device than the stream's");
    Op op;
    op.uses[0] = d.a;
    op.uses[1] = r.a;
    uint8_t* dp = static_cast<uint8_t*>(dst);
    const uint8_t* sp = static_cast<const uint8_t*>(src);
    op.fn = [=] {
        for (size_t k = 0; k < rows; ++k) std::memcpy(dp + k * dpitch, sp + k * spitch, width);
    };
    StandinOp lo{};
    lo.type = StandinOp::Copy;
    lo.kind = kind;
    lo.stream = unsigned(s - g_streams);
    lo.dst_alloc = alloc_number(d.a);
    lo.src_alloc = alloc_number(r.a);
    // pageable memory has no base: its offsets are the addresses
    lo.dst_off = reinterpret_cast<uintptr_t>(dst) - (d.a ? d.a->base.load(R) : 0);
    lo.src_off = reinterpret_cast<uintptr_t>(src) - (r.a ? r.a->base.load(R) : 0);
    lo.width = width;
    lo.rows = rows;
    lo.dpitch = dpitch;
    lo.spitch = spitch;
    const unsigned gen = s->gen.load(R);
    const uint64_t pos = enqueue(s, std::move(op));
    lo.pos = pos;
    log_op(lo);
    // pageable host memory on either side: the call returns once the copy is done
    if (!d.a || !r.a) wait_pos(s, gen, pos);
    return hipSuccess;
}

hipError_t alloc(void** out, size_t bytes, int kind, int idx, const char* call) {
    if (!out) return fail(hipErrorInvalidValue);
    *out = nullptr;
    if (injected(idx)) return fail(hipErrorOutOfMemory);
    if (bytes == 0) return hipSuccess;
    const size_t i = g_nallocs.fetch_add(1, R);
    if (i >= kMaxAllocs) {
        std::fprintf(stderr, "standin: allocation table full\n");
        std::abort();
    }
    void* raw = std::malloc(bytes + kAlign);
    if (!raw) return fail(hipErrorOutOfMemory);
    std::memset(raw, 0xEE, bytes + kAlign);  // fresh memory is not zero
    Alloc& a = g_allocs[i];
    a.raw.store(raw, R);
    a.base.store((reinterpret_cast<uintptr_t>(raw) + kAlign - 1) / kAlign * kAlign, R);
    a.size.store(bytes, R);
    a.device.store(t_device, R);
    a.pending.store(0, R);
    a.live.store(1, R);
    a.kind.store(kind, R);
    *out = reinterpret_cast<void*>(a.base.load(R));
    (void)call;
    return hipSuccess;
}

hipError_t release(void* p, int kind, const char* call) {
    if (!p) return hipSuccess;
    Alloc* a = find_alloc(p);
    if (!a || a->kind.load(R) != kind || reinterpret_cast<uintptr_t>(p) != a->base.load(R)) {
        violation(call, "a pointer this call never returned");
        return fail(hipErrorInvalidValue);
    }
    if (!a->live.exchange(0, R)) {
        violation(call, "double free of allocation #" + std::to_string(alloc_number(a)));
        return fail(hipErrorInvalidValue);
    }
    if (a->pending.load(R) != 0) {
        hazard(call, "allocation #" + std::to_string(alloc_number(a)) + " of " +
                         std::to_string(a->size.load(R)) + " bytes freed with queued work that names it");
        // as the real call does, wait for that work.  Only this path reads the counter with
        // acquire: a free that finds it zero gets no edge from the stream threads, so a free the
        // project did not order behind its copies stays a race for ThreadSanitizer.
        while (a->pending.load(std::memory_order_acquire) != 0)
            std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    if (kind == kDevice && a->device.load(R) != t_device)
        violation(call, "device memory of device " + std::to_string(a->device.load(R)) +
                            " freed with device " + std::to_string(t_device) + " current");
    std::memset(p, 0xDD, a->size.load(R));
    ASAN_POISON_MEMORY_REGION(p, a->size.load(R));
    return hipSuccess;
}

}  // namespace

const char* const standin_creating_calls[5] = {"hipMalloc", "hipHostMalloc",
                                               "hipStreamCreateWithFlags",
                                               "hipStreamCreateWithPriority",
                                               "hipEventCreateWithFlags"};

// ------------------------------------------------------------------------------------------
// The HIP calls
// ------------------------------------------------------------------------------------------
extern "C" {

hipError_t hipMalloc(void** ptr, size_t bytes) { return alloc(ptr, bytes, kDevice, 0, "hipMalloc"); }
hipError_t hipFree(void* ptr) { return release(ptr, kDevice, "hipFree"); }
hipError_t hipHostMalloc(void** ptr, size_t bytes, unsigned) {
    return alloc(ptr, bytes, kPinned, 1, "hipHostMalloc");
}
hipError_t hipHostFree(void* ptr) { return release(ptr, kPinned, "hipHostFree"); }

hipError_t hipMemset(void* dst, int value, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    const Side d = side_of(dst, bytes, "hipMemset", "destination");
    if (!d.a || !d.device) {
        violation("hipMemset", "destination is not device memory");
        return fail(hipErrorInvalidValue);
    }
    if (d.bad) return fail(hipErrorInvalidValue);
    std::memset(dst, value, bytes);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                          hipStream_t stream) {
    return copy2d("hipMemcpyAsync", dst, bytes, src, bytes, bytes, bytes ? 1 : 0, kind, stream);
}

hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                            size_t height, hipMemcpyKind kind, hipStream_t stream) {
    return copy2d("hipMemcpy2DAsync", dst, dpitch, src, spitch, width, height, kind, stream);
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned) {
    return make_stream(stream, 0, 2);
}
hipError_t hipStreamCreateWithPriority(hipStream_t* stream, unsigned, int priority) {
    return make_stream(stream, priority, 3);
}
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) {
    if (least) *least = 0;
    if (greatest) *greatest = -1;  // numerically lower = greater priority
    return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t stream) {
    ihipStream_t* s = stream_ok(stream, "hipStreamDestroy");
    if (!s) return fail(hipErrorInvalidResourceHandle);
    if (s->device.load(R) != t_device)
        violation("hipStreamDestroy", "stream of device " + std::to_string(s->device.load(R)) +
                                          " destroyed with device " + std::to_string(t_device) +
                                          " current");
    if (s->done.load(R) != s->enq.load(R))
        hazard("hipStreamDestroy", "stream #" + std::to_string(s - g_streams) + " destroyed with " +
                                       std::to_string(s->enq.load(R) - s->done.load(R)) +
                                       " operations still queued");
    {
        std::lock_guard<std::mutex> lk(s->mu);
        s->quit = true;
        s->held = false;  // the runtime lets queued work finish, then releases the stream
        s->cv.notify_all();
    }
    s->th.join();
    s->state.store(2, R);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        s->cv.notify_all();
    }
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t stream) {
    ihipStream_t* s = stream_ok(stream, "hipStreamSynchronize");
    if (!s) return fail(hipErrorInvalidResourceHandle);
    wait_pos(s, s->gen.load(R), s->enq.load(R));
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned) {
    ihipStream_t* s = stream_ok(stream, "hipStreamWaitEvent");
    ihipEvent_t* e = event_ok(event, "hipStreamWaitEvent");
    if (!s || !e) return fail(hipErrorInvalidResourceHandle);
    ihipStream_t* from = e->stream.load(R);
    StandinOp lo{};
    lo.type = StandinOp::WaitEvent;
    lo.stream = unsigned(s - g_streams);
    if (!from || from == s || g_mutant.load(R) == kMutantDropStreamWaitEvent) {
        lo.pos = s->enq.load(R);
        log_op(lo);
        return hipSuccess;  // never recorded, or in-order behind it already
    }
    const unsigned gen = e->gen.load(R);
    const uint64_t pos = e->pos.load(R);
    Op op;
    op.fn = [=] { wait_pos(from, gen, pos); };
    lo.pos = enqueue(s, std::move(op));
    log_op(lo);
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned) {
    if (!event) return fail(hipErrorInvalidValue);
    if (injected(4)) return fail(hipErrorOutOfMemory);
    const size_t i = g_nevents.fetch_add(1, R);
    if (i >= kMaxEvents) {
        std::fprintf(stderr, "standin: event table full\n");
        std::abort();
    }
    ihipEvent_t* e = &g_events[i];
    e->device.store(t_device, R);
    e->stream.store(nullptr, R);
    e->state.store(1, R);
    *event = e;
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t event) {
    ihipEvent_t* e = event_ok(event, "hipEventDestroy");
    if (!e) return fail(hipErrorInvalidResourceHandle);
    if (e->device.load(R) != t_device)
        violation("hipEventDestroy", "event of device " + std::to_string(e->device.load(R)) +
                                         " destroyed with device " + std::to_string(t_device) +
                                         " current");
    e->state.store(2, R);
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    ihipEvent_t* e = event_ok(event, "hipEventRecord");
    ihipStream_t* s = stream_ok(stream, "hipEventRecord");
    if (!e || !s) return fail(hipErrorInvalidResourceHandle);
    if (e->device.load(R) != s->device.load(R)) {
        violation("hipEventRecord", "event and stream of different devices");
        return fail(hipErrorInvalidResourceHandle);
    }
    uint64_t pos;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        pos = s->enq.load(R);
    }
    e->gen.store(s->gen.load(R), R);
    e->pos.store(pos, R);
    e->stream.store(s, R);
    StandinOp lo{};
    lo.type = StandinOp::EventRecord;
    lo.stream = unsigned(s - g_streams);
    lo.pos = pos;
    log_op(lo);
    return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t event) {
    ihipEvent_t* e = event_ok(event, "hipEventSynchronize");
    if (!e) return fail(hipErrorInvalidResourceHandle);
    ihipStream_t* s = e->stream.load(R);
    if (!s || g_mutant.load(R) == kMutantEventSyncNoWait) return hipSuccess;
    wait_pos(s, e->gen.load(R), e->pos.load(R));
    return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t event) {
    ihipEvent_t* e = event_ok(event, "hipEventQuery");
    if (!e) return fail(hipErrorInvalidResourceHandle);
    ihipStream_t* s = e->stream.load(R);
    if (!s || reached(s, e->gen.load(R), e->pos.load(R))) return hipSuccess;
    return hipErrorNotReady;
}

hipError_t hipGetDevice(int* device) {
    if (!device) return fail(hipErrorInvalidValue);
    *device = t_device;
    return hipSuccess;
}
hipError_t hipSetDevice(int device) {
    if (device < 0 || device >= g_devices.load(R)) return fail(hipErrorInvalidDevice);
    t_device = device;
    return hipSuccess;
}
hipError_t hipGetDeviceCount(int* count) {
    if (!count) return fail(hipErrorInvalidValue);
    *count = g_devices.load(R);
    return hipSuccess;
}
hipError_t hipGetLastError(void) {
    const hipError_t e = t_error;
    t_error = hipSuccess;
    return e;
}
const char* hipGetErrorString(hipError_t e) {
    switch (e) {
        case hipSuccess: return "no error";
        case hipErrorInvalidValue: return "invalid argument";
        case hipErrorOutOfMemory: return "out of memory";
        case hipErrorInvalidDevice: return "invalid device ordinal";
        case hipErrorInvalidResourceHandle: return "invalid resource handle";
        case hipErrorNotReady: return "device not ready";
        default: return "operation not supported";
    }
}

hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attr, const void* ptr) {
    if (!attr) return fail(hipErrorInvalidValue);
    Alloc* a = find_alloc(ptr);
    if (!a || !a->live.load(R)) return fail(hipErrorInvalidValue);  // pageable memory
    const bool dev = a->kind.load(R) == kDevice;
    attr->type = dev ? hipMemoryTypeDevice : hipMemoryTypeHost;
    attr->device = a->device.load(R);
    attr->devicePointer = const_cast<void*>(ptr);
    attr->hostPointer = dev ? nullptr : const_cast<void*>(ptr);
    return hipSuccess;
}

hipError_t hipPointerGetAttribute(void* data, hipPointer_attribute attr, hipDeviceptr_t ptr) {
    if (!data) return fail(hipErrorInvalidValue);
    Alloc* a = find_alloc(ptr);
    if (!a || !a->live.load(R)) return fail(hipErrorInvalidValue);
    if (attr == HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR)
        *static_cast<void**>(data) = reinterpret_cast<void*>(a->base.load(R));
    else if (attr == HIP_POINTER_ATTRIBUTE_RANGE_SIZE)
        *static_cast<size_t*>(data) = a->size.load(R);
    else
        return fail(hipErrorInvalidValue);
    return hipSuccess;
}

hipError_t hipDeviceGetPCIBusId(char*, int, int) { return fail(hipErrorNotSupported); }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// The test's side
// ------------------------------------------------------------------------------------------
void standin_reset() {
    const StandinLive live = standin_live();
    if (live.total()) {
        std::fprintf(stderr, "standin_reset with %zu objects live\n", live.total());
        std::abort();
    }
    const size_t na = std::min(g_nallocs.load(R), kMaxAllocs);
    for (size_t i = 0; i < na; ++i) {
        ASAN_UNPOISON_MEMORY_REGION(reinterpret_cast<void*>(g_allocs[i].base.load(R)),
                                    g_allocs[i].size.load(R));
        std::free(g_allocs[i].raw.exchange(nullptr, R));
        g_allocs[i].kind.store(kNone, R);
        g_allocs[i].base.store(0, R);
        g_allocs[i].size.store(0, R);
    }
    g_nallocs.store(0, R);
    const size_t ns = std::min(g_nstreams.load(R), kMaxStreams);
    for (size_t i = 0; i < ns; ++i) g_streams[i].state.store(0, R);
    g_nstreams.store(0, R);
    const size_t ne = std::min(g_nevents.load(R), kMaxEvents);
    for (size_t i = 0; i < ne; ++i) g_events[i].state.store(0, R);
    g_nevents.store(0, R);
    g_nops.store(0, R);
    g_log.store(false, R);
    g_devices.store(1, R);
    g_seed.store(0, R);
    g_mutant.store(0, R);
    t_device = 0;
    t_error = hipSuccess;
    standin_clear_calls();
    std::lock_guard<std::mutex> lk(g_list_mu);
    g_violations.clear();
    g_hazards.clear();
}

void standin_set_devices(int n) { g_devices.store(n, R); }
void standin_set_seed(uint64_t seed) { g_seed.store(seed, R); }
void standin_set_mutant(StandinMutant m) { g_mutant.store(int(m), R); }

static void set_held(ihipStream_t* s, bool held) {
    std::lock_guard<std::mutex> lk(s->mu);
    s->held = held;
    s->cv.notify_all();
}
void standin_hold(hipStream_t s) {
    if (stream_ok(s, "standin_hold")) set_held(s, true);
}
void standin_release(hipStream_t s) {
    if (stream_ok(s, "standin_release")) set_held(s, false);
}
void standin_hold_all() {
    for (hipStream_t s : standin_streams()) set_held(s, true);
}
void standin_release_all() {
    for (hipStream_t s : standin_streams()) set_held(s, false);
}
std::vector<hipStream_t> standin_streams() {
    std::vector<hipStream_t> v;
    const size_t n = std::min(g_nstreams.load(R), kMaxStreams);
    for (size_t i = 0; i < n; ++i)
        if (g_streams[i].state.load(R) == 1) v.push_back(&g_streams[i]);
    return v;
}
uint64_t standin_stream_launches(hipStream_t s) { return s->launches.load(R); }
unsigned standin_stream_number(hipStream_t s) { return unsigned(s - g_streams); }

hipError_t standin_enqueue(hipStream_t stream, const char* label, std::function<void()> fn,
                           const std::vector<const void*>& uses) {
    ihipStream_t* s = stream_ok(stream, label);
    if (!s) return fail(hipErrorInvalidResourceHandle);
    Op op;
    op.launch = true;
    size_t n = 0;
    for (const void* p : uses) {
        Alloc* a = find_alloc(p);
        if (!a || a->kind.load(R) != kDevice || !a->live.load(R)) {
            violation(label, "a launch argument that is not live device memory");
            continue;
        }
        if (a->device.load(R) != s->device.load(R))
            violation(label, "device memory of another device than the stream's");
        if (n < 4) op.uses[n++] = a;
    }
    op.fn = std::move(fn);
    StandinOp lo{};
    lo.type = StandinOp::Launch;
    lo.stream = unsigned(s - g_streams);
    lo.label = label;
    lo.pos = enqueue(s, std::move(op));
    log_op(lo);
    return hipSuccess;
}

void standin_check_device_range(const void* p, size_t n, const char* what) {
    const Side s = side_of(p, n, what, "range");
    if (!s.a || !s.device) violation(what, "not device memory");
    // the compute stand-ins go on to touch the range: a breach ends the run here
    if (!s.a || !s.device || s.bad) {
        for (const std::string& v : standin_violations()) std::fprintf(stderr, "violation: %s\n", v.c_str());
        std::fprintf(stderr, "FAILED: a launch names memory outside a live device allocation\n");
        std::fflush(stderr);
        std::_Exit(1);
    }
}

void standin_fail(const char* name, uint64_t nth) {
    const int i = call_index(name);
    g_fail_at[i].store(nth ? g_calls[i].load(R) + nth : 0, R);
}
uint64_t standin_calls(const char* name) { return g_calls[call_index(name)].load(R); }
void standin_clear_calls() {
    for (int i = 0; i < 5; ++i) {
        g_calls[i].store(0, R);
        g_fail_at[i].store(0, R);
    }
}

std::vector<std::string> standin_violations() {
    std::lock_guard<std::mutex> lk(g_list_mu);
    return g_violations;
}
std::vector<std::string> standin_hazards() {
    std::lock_guard<std::mutex> lk(g_list_mu);
    return g_hazards;
}

StandinLive standin_live() {
    StandinLive l{};
    const size_t na = std::min(g_nallocs.load(R), kMaxAllocs);
    for (size_t i = 0; i < na; ++i)
        if (g_allocs[i].live.load(R))
            ++(g_allocs[i].kind.load(R) == kDevice ? l.device_allocs : l.pinned_allocs);
    const size_t ns = std::min(g_nstreams.load(R), kMaxStreams);
    for (size_t i = 0; i < ns; ++i) l.streams += g_streams[i].state.load(R) == 1;
    const size_t ne = std::min(g_nevents.load(R), kMaxEvents);
    for (size_t i = 0; i < ne; ++i) l.events += g_events[i].state.load(R) == 1;
    return l;
}

void standin_log(bool on) { g_log.store(on, R); }
std::vector<StandinOp> standin_ops() {
    const size_t n = std::min(g_nops.load(R), kMaxOps);
    return std::vector<StandinOp>(g_ops, g_ops + n);
}
int standin_alloc_of(const void* p) { return alloc_number(find_alloc(p)); }
