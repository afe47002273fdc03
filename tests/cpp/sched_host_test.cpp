// The scheduler (csrc/multi.cpp), the write and read pipelines (csrc/pipeline.cpp) and the pinned
// registry (csrc/hostmem.cpp) run unchanged on the CPU: linked against the host HIP stand-in
// (hip_standin/) and the oracle-backed compute stand-ins (sched_host_compute.cpp).  Streams are
// real threads with seeded delays, so a missing wait, a buffer freed under queued work, a handle
// used after its destruction or a race between a worker and the destroying thread shows here (as a
// result mismatch, a stand-in violation or hazard, or a sanitizer report) where a GPU hides it or
// faults.  Expected results come from the oracle over whole jobs; every caller output lies
// between canaries.
//
//   sched_host_test [first_seed [n_seeds]]
// SCHED_HOST_MUTANT=event_sync | stream_wait breaks the stand-in on purpose (the wrapper requires
// a non-zero exit then); SCHED_HOST_ONLY=<letters of a..e, s for the self-test> picks scenarios.
#include <hip/hip_runtime.h>
#include <dirent.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "chunky_ec.h"
#include "hip_standin/standin.hpp"
#include "pipeline_internal.hpp"

extern "C" {
void or_sha256(const uint8_t* buf, size_t len, uint8_t out[32]);
int or_rs_encode_sep(size_t d, size_t p, const uint8_t* const* data, const size_t* data_lens,
                     size_t n_data, uint8_t* const* parity, const size_t* parity_lens,
                     size_t n_parity);
}

#if defined(__SANITIZE_THREAD__)
// libstdc++'s condition_variable::wait_for (the scheduler's worker loop) waits with
// pthread_cond_clockwait, which older ThreadSanitizer runtimes do not intercept: they miss the
// unlock and relock inside the wait and report a double lock of the scheduler's mutex.  Under
// ThreadSanitizer the call is routed to pthread_cond_timedwait, which every runtime intercepts.
#include <pthread.h>
#include <time.h>
extern "C" int pthread_cond_clockwait(pthread_cond_t* cond, pthread_mutex_t* mutex, clockid_t clock,
                                      const struct timespec* abstime) {
    struct timespec now{}, real{};
    clock_gettime(clock, &now);
    clock_gettime(CLOCK_REALTIME, &real);
    long long ns = (abstime->tv_sec - now.tv_sec) * 1000000000ll + (abstime->tv_nsec - now.tv_nsec);
    if (ns < 0) ns = 0;
    ns += real.tv_sec * 1000000000ll + real.tv_nsec;
    struct timespec until{time_t(ns / 1000000000ll), long(ns % 1000000000ll)};
    return pthread_cond_timedwait(cond, mutex, &until);
}
#endif

namespace {

std::string g_where;  // scenario and parameters, for messages
std::atomic<uint64_t> g_checks{0};  // relaxed: a count, no ordering between the test's threads

[[noreturn]] void die(const char* file, int line, const char* fmt, ...) {
    std::printf("FAILED %s:%d [%s]: ", file, line, g_where.c_str());
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
    for (const std::string& v : standin_violations()) std::printf("  violation: %s\n", v.c_str());
    for (const std::string& v : standin_hazards()) std::printf("  hazard: %s\n", v.c_str());
    std::fflush(stdout);
    _exit(1);  // streams and workers may still be running
}
#define CHECK(cond, ...)                                  \
    do {                                                  \
        g_checks.fetch_add(1, std::memory_order_relaxed);  \
        if (!(cond)) die(__FILE__, __LINE__, __VA_ARGS__); \
    } while (0)

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 12345) {}
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t x = s;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    }
    size_t below(size_t n) { return size_t(next() % n); }
};

void sleep_us(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

size_t thread_count() {
    size_t n = 0;
    if (DIR* dir = opendir("/proc/self/task")) {
        while (dirent* e = readdir(dir)) n += e->d_name[0] != '.';
        closedir(dir);
    }
    return n;
}
size_t g_base_threads = 0;

// A caller buffer between canaries, pageable or page-locked (cec_host_alloc).
constexpr size_t kGuard = 64;
struct Buf {
    uint8_t* raw = nullptr;
    size_t n = 0;
    bool pinned = false;
    Buf(size_t bytes, bool pin, int device = 0) : n(bytes), pinned(pin) {
        if (pinned) {
            void* p = nullptr;
            CHECK(cec_host_alloc(n + 2 * kGuard, device, &p) == CEC_OK, "cec_host_alloc");
            raw = static_cast<uint8_t*>(p);
        } else {
            raw = static_cast<uint8_t*>(std::malloc(n + 2 * kGuard));
        }
        std::memset(raw, 0xC5, n + 2 * kGuard);
        std::memset(raw + kGuard, 0xA7, n);
    }
    Buf(const Buf&) = delete;
    ~Buf() {
        if (pinned) cec_host_free(raw);
        else std::free(raw);
    }
    uint8_t* p() { return raw + kGuard; }
    void check(const char* what) {
        for (size_t i = 0; i < kGuard; ++i)
            CHECK(raw[i] == 0xC5 && raw[kGuard + n + i] == 0xC5, "canary of %s overwritten", what);
    }
};
using BufP = std::unique_ptr<Buf>;
BufP buf(size_t n, bool pin, int device = 0) { return std::make_unique<Buf>(n, pin, device); }

// n parts of RS(d,p) with chunk length L, encoded and hashed by the oracle.
struct Fix {
    size_t d, p, t, L, n;
    std::vector<uint8_t> data, parity, chunks, dig;
    const uint8_t* chunk(size_t k, size_t i) const { return chunks.data() + (k * t + i) * L; }
};
Fix make_fix(size_t d, size_t p, size_t L, size_t n, uint64_t seed) {
    Fix f{d, p, d + p, L, n, {}, {}, {}, {}};
    f.data.resize(n * d * L);
    f.parity.resize(n * p * L);
    f.chunks.resize(n * f.t * L);
    f.dig.resize(n * f.t * 32);
    Rng r(seed ^ 0xF1Cull);
    for (size_t i = 0; i < f.data.size(); i += 8) {
        const uint64_t x = r.next();
        std::memcpy(f.data.data() + i, &x, std::min<size_t>(8, f.data.size() - i));
    }
    std::vector<const uint8_t*> dp(d);
    std::vector<uint8_t*> pp(p);
    const std::vector<size_t> dl(d, L), pl(p, L);
    for (size_t k = 0; k < n; ++k) {
        for (size_t j = 0; j < d; ++j) dp[j] = f.data.data() + (k * d + j) * L;
        for (size_t i = 0; i < p; ++i) pp[i] = f.parity.data() + (k * p + i) * L;
        CHECK(or_rs_encode_sep(d, p, dp.data(), dl.data(), d, pp.data(), pl.data(), p) == 0,
              "oracle encode");
        std::memcpy(f.chunks.data() + k * f.t * L, f.data.data() + k * d * L, d * L);
        std::memcpy(f.chunks.data() + (k * f.t + d) * L, f.parity.data() + k * p * L, p * L);
        for (size_t i = 0; i < f.t; ++i) or_sha256(f.chunk(k, i), L, f.dig.data() + (k * f.t + i) * 32);
    }
    return f;
}

// What a reader loaded of one part.  Kinds: 0 every chunk; 1 exactly d chunks, data chunks among
// the missing; 2 d+1 chunks, one of them damaged (decoded again inside wait); 3 the d data chunks,
// chunk 0 damaged: d-1 verify, TooFewShardsPresent (its retry: retry_of_kind3).
struct Loaded {
    std::vector<uint8_t> present;  // [t]
    int damaged = -1;
};
Loaded load_kind(int kind, size_t d, size_t t, Rng& r) {
    Loaded l;
    l.present.assign(t, 0);
    if (kind == 0) {
        std::fill(l.present.begin(), l.present.end(), 1);
    } else if (kind == 3) {
        for (size_t i = 0; i < d; ++i) l.present[i] = 1;
        l.damaged = 0;
    } else {
        const size_t want = kind == 1 ? d : d + 1;
        const size_t skip = r.below(t);  // a run of missing chunks starting anywhere
        for (size_t i = 0, have = 0; i < t && have < want; ++i) {
            const size_t x = (skip + 1 + i) % t;
            l.present[x] = uint8_t(1 + r.below(3));  // any nonzero flag means loaded
            ++have;
        }
        if (kind == 2) {
            do l.damaged = int(r.below(t));
            while (!l.present[size_t(l.damaged)]);
        }
    }
    return l;
}

// One read job (or batch): inputs in the [n][t][L] layout, expectations from the fixture.
struct ReadCase {
    size_t d, t, L, n;
    std::vector<size_t> part;     // fixture part of each job part
    std::vector<uint8_t> present, expected;
    std::vector<int> damaged;     // per part, -1 none
    std::vector<uint8_t> chunks;  // [n][t][L]; chunks not loaded (or carried) hold 0x5A
    std::vector<uint8_t> want_ok;
    std::vector<int> want_status;  // read / resilver status
};
ReadCase make_read(const Fix& f, const std::vector<size_t>& parts, const std::vector<int>& kinds,
                   Rng& r) {
    ReadCase c{f.d, f.t, f.L, parts.size(), parts, {}, {}, {}, {}, {}, {}};
    const size_t t = f.t, L = f.L;
    c.present.resize(c.n * t);
    c.expected.resize(c.n * t * 32);
    c.chunks.assign(c.n * t * L, 0x5A);
    c.want_ok.assign(c.n * t, 0);
    c.want_status.assign(c.n, CEC_OK);
    c.damaged.assign(c.n, -1);
    for (size_t k = 0; k < c.n; ++k) {
        const Loaded l = load_kind(kinds[k], f.d, t, r);
        c.damaged[k] = l.damaged;
        std::memcpy(c.expected.data() + k * t * 32, f.dig.data() + parts[k] * t * 32, t * 32);
        size_t good = 0;
        for (size_t i = 0; i < t; ++i) {
            c.present[k * t + i] = l.present[i];
            if (!l.present[i]) continue;
            uint8_t* to = c.chunks.data() + (k * t + i) * L;
            std::memcpy(to, f.chunk(parts[k], i), L);
            if (int(i) == l.damaged) to[r.below(L)] ^= 0x40;
            else c.want_ok[k * t + i] = 1, ++good;
        }
        if (good < f.d) c.want_status[k] = CEC_TOO_FEW_SHARDS_PRESENT;
    }
    return c;
}
// The retry of a kind-3 part k of `c`: its verified chunks flagged CEC_PRESENT_VERIFIED (their
// bytes NOT supplied: they come from the carry pool), chunk 0 dropped, the first parity chunk new.
void retry_of_kind3(ReadCase& c, size_t k, const Fix& f) {
    const size_t t = c.t, L = c.L, d = c.d;
    c.present[k * t] = 0;
    c.damaged[k] = -1;
    for (size_t i = 1; i < d; ++i) {
        c.present[k * t + i] = CEC_PRESENT_VERIFIED;
        std::memset(c.chunks.data() + (k * t + i) * L, 0x5A, L);
        c.want_ok[k * t + i] = 1;
    }
    std::memset(c.chunks.data() + k * t * L, 0x5A, L);
    c.want_ok[k * t] = 0;
    c.present[k * t + d] = 1;
    std::memcpy(c.chunks.data() + (k * t + d) * L, f.chunk(c.part[k], d), L);
    c.want_ok[k * t + d] = 1;
    c.want_status[k] = CEC_OK;
}

void check_verified(const ReadCase& c, const uint8_t* ver, const char* what) {
    for (size_t x = 0; x < c.n * c.t; ++x)
        CHECK((ver[x] != 0) == (c.want_ok[x] != 0),
              "result mismatch: %s verified flag of part %zu chunk %zu is %d", what, x / c.t,
              x % c.t, int(ver[x]));
}
// ptrs: [n][W] chunk locations (W = d: the data chunks; W = t: resilver).
void check_chunks(const ReadCase& c, const Fix& f, const int* status, const uint8_t* const* ptrs,
                  size_t W, const char* what) {
    for (size_t k = 0; k < c.n; ++k) {
        CHECK(status[k] == c.want_status[k], "result mismatch: %s status of part %zu is %d, not %d",
              what, k, status[k], c.want_status[k]);
        if (status[k] != CEC_OK) continue;
        for (size_t j = 0; j < W; ++j) {
            const uint8_t* got = ptrs[k * W + j];
            CHECK(got != nullptr, "result mismatch: %s part %zu chunk %zu has no location", what, k, j);
            CHECK(std::memcmp(got, f.chunk(c.part[k], j), c.L) == 0,
                  "result mismatch: %s part %zu chunk %zu has wrong bytes", what, k, j);
        }
    }
}

void begin(const char* fmt, ...) {
    char b[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    g_where = b;
    standin_reset();
}
void set_schedule(uint64_t seed, StandinMutant mutant) {
    standin_set_seed(seed);
    standin_set_mutant(mutant);
}
StandinMutant g_mutant = kMutantNone;

// Every stream live now (one per slot of every pipeline) has run at least one launch: a scenario
// cannot pass by doing nothing.
void check_slots_used() {
    for (hipStream_t s : standin_streams())
        CHECK(standin_stream_launches(s) > 0, "the slot of stream #%u carried no batch",
              standin_stream_number(s));
}
void check_clean(const char* when) {
    const auto v = standin_violations(), h = standin_hazards();
    CHECK(v.empty(), "%zu stand-in violations %s", v.size(), when);
    CHECK(h.empty(), "%zu stand-in hazards %s", h.size(), when);
}
void finish() {
    check_clean("at the end of the scenario");
    const StandinLive l = standin_live();
    CHECK(l.total() == 0, "left live: %zu device, %zu pinned allocations, %zu streams, %zu events",
          l.device_allocs, l.pinned_allocs, l.streams, l.events);
    // a joined thread's entry under /proc/self/task goes a moment after the join returns
    size_t threads = thread_count();
    for (int spin = 0; threads > g_base_threads && spin < 500; ++spin) {
        sleep_us(1000);
        threads = thread_count();
    }
    CHECK(threads <= g_base_threads, "%zu threads left running", threads - g_base_threads);
}

// ------------------------------------------------------------------------------------------
// Self-test of the stand-in
// ------------------------------------------------------------------------------------------
void standin_selftest() {
    begin("selftest");
    standin_set_devices(2);
    auto nv = [] { return standin_violations().size(); };
    auto nh = [] { return standin_hazards().size(); };
    hipStream_t s1 = nullptr, s2 = nullptr;
    hipEvent_t e = nullptr;
    CHECK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking) == hipSuccess, "stream");
    CHECK(hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, -1) == hipSuccess, "stream");
    CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess, "event");
    void *dev = nullptr, *pin = nullptr;
    CHECK(hipMalloc(&dev, 1000) == hipSuccess && hipHostMalloc(&pin, 1500, 0) == hipSuccess, "alloc");
    std::vector<uint8_t> page(1000, 7);

    // events capture a position; a held stream runs nothing; waits wait for what they name
    std::atomic<int> a{0}, b{0}, b_saw_a{-1};
    CHECK(hipEventQuery(e) == hipSuccess, "an event never recorded is complete");
    standin_hold(s1);
    CHECK(standin_enqueue(s1, "a", [&] { a = 1; }, {}) == hipSuccess, "enqueue");
    CHECK(hipEventRecord(e, s1) == hipSuccess, "record");
    CHECK(standin_enqueue(s1, "b", [&] { sleep_us(2000); b = 1; }, {}) == hipSuccess, "enqueue");
    CHECK(hipStreamWaitEvent(s2, e, 0) == hipSuccess, "wait event");
    CHECK(standin_enqueue(s2, "c", [&] { b_saw_a = a.load(); }, {}) == hipSuccess, "enqueue");
    sleep_us(3000);
    CHECK(hipEventQuery(e) == hipErrorNotReady, "query on a held stream");
    CHECK(hipGetLastError() == hipSuccess, "hipErrorNotReady is not sticky");
    CHECK(a == 0 && b_saw_a == -1, "a held stream ran, or a stream ran past hipStreamWaitEvent");
    standin_release(s1);
    CHECK(hipEventSynchronize(e) == hipSuccess && a == 1, "hipEventSynchronize waits for its position");
    CHECK(hipEventQuery(e) == hipSuccess, "query after synchronize");
    CHECK(hipStreamSynchronize(s2) == hipSuccess && b_saw_a == 1, "hipStreamWaitEvent orders streams");
    CHECK(hipStreamSynchronize(s1) == hipSuccess && b == 1, "hipStreamSynchronize waits for the queue");
    // the position is the one at the record: work queued later does not reopen the event
    standin_hold(s1);
    CHECK(standin_enqueue(s1, "d", [] {}, {}) == hipSuccess, "enqueue");
    CHECK(hipEventQuery(e) == hipSuccess, "an event is complete at its captured position");
    standin_release(s1);
    // a pageable copy blocks; a pinned one is asynchronous
    std::memset(dev, 3, 1000);
    standin_set_seed(5);
    CHECK(hipMemcpyAsync(page.data(), dev, 1000, hipMemcpyDeviceToHost, s1) == hipSuccess, "copy");
    CHECK(page[0] == 3 && page[999] == 3, "a pageable copy returns when it is done");
    standin_set_seed(0);
    standin_hold(s1);
    std::memset(pin, 0, 1000);
    CHECK(hipMemcpy2DAsync(pin, 100, dev, 200, 50, 5, hipMemcpyDeviceToHost, s1) == hipSuccess, "copy");
    CHECK(static_cast<uint8_t*>(pin)[0] == 0, "a pinned copy on a held stream has not run");
    standin_release(s1);
    CHECK(hipStreamSynchronize(s1) == hipSuccess, "sync");
    CHECK(static_cast<uint8_t*>(pin)[449] == 3 && static_cast<uint8_t*>(pin)[450] == 0 &&
              static_cast<uint8_t*>(pin)[50] == 0, "2-D copy geometry");
    // pointer queries, the sticky per-thread error
    hipPointerAttribute_t at{};
    CHECK(hipPointerGetAttributes(&at, page.data()) == hipErrorInvalidValue, "pageable pointer");
    CHECK(hipGetLastError() == hipErrorInvalidValue && hipGetLastError() == hipSuccess, "sticky error");
    CHECK(hipPointerGetAttributes(&at, static_cast<uint8_t*>(pin) + 10) == hipSuccess &&
              at.type == hipMemoryTypeHost, "pinned pointer");
    size_t range = 0;
    void* start = nullptr;
    CHECK(hipPointerGetAttribute(&range, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, pin) == hipSuccess &&
              range == 1500, "range size");
    CHECK(hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR,
                                 static_cast<uint8_t*>(pin) + 10) == hipSuccess && start == pin,
          "range start");
    CHECK(hipPointerGetAttributes(&at, dev) == hipSuccess && at.type == hipMemoryTypeDevice, "device");
    std::thread([&] {
        int dv = -1;
        CHECK(hipGetLastError() == hipSuccess && hipGetDevice(&dv) == hipSuccess && dv == 0,
              "errors and the current device are per thread");
    }).join();
    char bus[16];
    CHECK(hipDeviceGetPCIBusId(bus, 16, 0) != hipSuccess && hipGetLastError() != hipSuccess, "bus id");
    // fault injection
    void* x[3] = {};
    standin_clear_calls();
    standin_fail("hipMalloc", 2);
    CHECK(hipMalloc(&x[0], 8) == hipSuccess && hipMalloc(&x[1], 8) == hipErrorOutOfMemory &&
              hipMalloc(&x[2], 8) == hipSuccess && !x[1] && standin_calls("hipMalloc") == 3,
          "the 2nd hipMalloc fails once");
    CHECK(hipGetLastError() == hipErrorOutOfMemory, "the failure is the thread's last error");
    CHECK(hipFree(x[0]) == hipSuccess && hipFree(x[2]) == hipSuccess, "free");
    CHECK(nv() == 0 && nh() == 0, "no violation so far");

    // one of each violation class
    size_t v = 0;
    auto one_more = [&](const char* what) {
        ++v;
        CHECK(nv() == v, "violation not recorded (or recorded twice): %s", what);
    };
    (void)hipMemcpyAsync(dev, pin, 1001, hipMemcpyHostToDevice, s1);
    one_more("device side past its allocation");
    (void)hipMemcpy2DAsync(dev, 10, pin, 150, 10, 11, hipMemcpyHostToDevice, s1);
    one_more("pinned side past its allocation");
    (void)hipMemcpyAsync(pin, dev, 8, hipMemcpyHostToDevice, s1);
    one_more("kind contradicts the pointers");
    (void)hipMemcpy2DAsync(dev, 8, pin, 16, 12, 2, hipMemcpyHostToDevice, s1);
    one_more("width > pitch");
    (void)hipMemset(static_cast<uint8_t*>(dev) + 990, 0, 20);
    one_more("memset past its allocation");
    (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(&page[0]));
    one_more("never-created stream");
    (void)hipStreamSynchronize(s1);
    hipStream_t s3 = nullptr;
    CHECK(hipStreamCreateWithFlags(&s3, 0) == hipSuccess && hipStreamDestroy(s3) == hipSuccess, "s3");
    (void)hipStreamSynchronize(s3);
    one_more("destroyed stream");
    (void)hipStreamDestroy(s3);
    one_more("stream destroyed twice");
    hipEvent_t e2 = nullptr;
    CHECK(hipEventCreateWithFlags(&e2, 0) == hipSuccess && hipEventDestroy(e2) == hipSuccess, "e2");
    (void)hipEventRecord(e2, s1);
    one_more("destroyed event");
    (void)hipEventDestroy(e2);
    one_more("event destroyed twice");
    void* y = nullptr;
    CHECK(hipMalloc(&y, 64) == hipSuccess && hipFree(y) == hipSuccess, "y");
    (void)hipFree(y);
    one_more("double free");
    (void)hipMemcpyAsync(y, pin, 8, hipMemcpyHostToDevice, s1);
    one_more("copy into freed device memory");
    CHECK(hipSetDevice(1) == hipSuccess && hipMalloc(&y, 64) == hipSuccess &&
              hipSetDevice(0) == hipSuccess, "device 1");
    (void)hipFree(y);
    one_more("device memory freed with another device current");
    (void)hipStreamSynchronize(s1);
    CHECK(nh() == 0, "no hazard so far");
    // hazards: a free and a stream destroy under queued work
    standin_hold(s1);
    CHECK(hipMemcpyAsync(dev, pin, 8, hipMemcpyHostToDevice, s1) == hipSuccess, "copy");
    std::thread rel([&] { sleep_us(2000); standin_release(s1); });
    CHECK(hipFree(dev) == hipSuccess && nh() == 1, "hipFree under a queued copy is a hazard");
    rel.join();
    standin_hold(s2);
    CHECK(standin_enqueue(s2, "e", [] {}, {}) == hipSuccess, "enqueue");
    CHECK(hipStreamDestroy(s2) == hipSuccess && nh() == 2, "hipStreamDestroy under queued work is a hazard");
    CHECK(nv() == v, "hazards are not violations");
    CHECK(hipStreamDestroy(s1) == hipSuccess && hipEventDestroy(e) == hipSuccess &&
              hipHostFree(pin) == hipSuccess, "cleanup");
    const StandinLive l = standin_live();
    CHECK(l.total() == 0, "selftest left %zu objects live", l.total());
    std::printf("selftest: ok (%zu violations and 2 hazards seeded and recorded)\n", v);
}

// ------------------------------------------------------------------------------------------
// a. Write pipeline
// ------------------------------------------------------------------------------------------
struct Codec {
    cec_codec* c = nullptr;
    Codec(size_t d, size_t p) { CHECK(cec_codec_new(d, p, &c) == CEC_OK, "codec"); }
    ~Codec() { cec_codec_free(c); }
};

void scenario_write(size_t d, size_t p, size_t L, size_t P, size_t depth, uint64_t seed) {
    begin("a write RS(%zu,%zu) L=%zu P=%zu depth=%zu seed=%llu", d, p, L, P, depth,
          (unsigned long long)seed);
    set_schedule(seed, g_mutant);
    const size_t t = d + p, cs = (L + 255) / 256 * 256, B = 3 * depth;
    Codec codec(d, p);
    cec_pipeline* pl = nullptr;
    CHECK(cec_pipeline_new_ex(codec.c, L, P, depth, 0u, &pl) == CEC_OK, "cec_pipeline_new_ex: %s",
          cec_pipeline_last_error());
    const std::vector<hipStream_t> streams = standin_streams();
    CHECK(streams.size() == depth && cec_pipeline_depth(pl) == depth, "one stream per slot");
    Rng r(seed);
    std::vector<size_t> nb(B), first(B);
    size_t total = 0;
    for (size_t b = 0; b < B; ++b) {
        nb[b] = b % 4 == 3 ? 1 + r.below(P - 1) : P;  // fewer parts than parts_per_batch too
        first[b] = total;
        total += nb[b];
    }
    const Fix f = make_fix(d, p, L, total, seed);
    standin_log(true);
    struct Pending {
        bool used = false;
        size_t b = 0;
        BufP in, par, dig;
    };
    std::vector<Pending> pend(depth);
    std::vector<std::vector<size_t>> slot_batches(depth);
    auto collect = [&](size_t slot) {
        Pending& q = pend[slot];
        const uint8_t *par = nullptr, *dig = nullptr;
        size_t got = 0;
        CHECK(cec_pipeline_wait(pl, slot, &par, &dig, &got) == CEC_OK, "wait");
        CHECK(cec_pipeline_query(pl, slot) == 1, "query after wait");
        CHECK(got == nb[q.b], "wait gives %zu parts, not %zu", got, nb[q.b]);
        if (q.par) CHECK(par == q.par->p(), "wait's parity is not where submit_from put it");
        if (q.dig) CHECK(dig == q.dig->p(), "wait's digests are not where submit_from put them");
        CHECK(std::memcmp(par, f.parity.data() + first[q.b] * p * L, got * p * L) == 0,
              "result mismatch: parity of batch %zu (slot %zu)", q.b, slot);
        CHECK(std::memcmp(dig, f.dig.data() + first[q.b] * t * 32, got * t * 32) == 0,
              "result mismatch: digests of batch %zu (slot %zu)", q.b, slot);
        for (Buf* x : {q.in.get(), q.par.get(), q.dig.get()})
            if (x) x->check("write batch buffer");
        q = Pending{};
    };
    for (size_t b = 0; b < B; ++b) {
        size_t slot = 0;
        uint8_t* data = nullptr;
        CHECK(cec_pipeline_acquire(pl, &slot, &data) == CEC_OK && data, "acquire");
        if (pend[slot].used) collect(slot);
        Pending& q = pend[slot];
        q.used = true;
        q.b = b;
        slot_batches[slot].push_back(b);
        const size_t n = nb[b];
        const uint8_t* src = f.data.data() + first[b] * d * L;
        const int mode = int(b % 3);  // slot buffers, caller pinned, caller pageable
        const bool hold = b == 0 || (mode == 1 && r.below(2));
        if (hold) standin_hold(streams[slot]);
        if (mode == 0) {
            std::memcpy(data, src, n * d * L);
            CHECK(cec_pipeline_submit(pl, slot, n) == CEC_OK, "submit: %s", cec_pipeline_last_error());
        } else {
            const bool pin = mode == 1;
            q.in = buf(n * d * L, pin);
            std::memcpy(q.in->p(), src, n * d * L);
            q.par = buf(n * p * L, pin);
            if (b % 2) q.dig = buf(n * t * 32, pin);  // else the slot's own digest buffer
            CHECK(cec_pipeline_submit_from(pl, slot, q.in->p(), n, q.par->p(),
                                           q.dig ? q.dig->p() : nullptr) == CEC_OK,
                  "submit_from: %s", cec_pipeline_last_error());
        }
        if (hold) {
            sleep_us(300);
            CHECK(cec_pipeline_query(pl, slot) == 0, "query is 0 while the slot's stream is held");
            std::thread rel([&] { sleep_us(1500); standin_release(streams[slot]); });
            collect(slot);  // wait must wait for the release
            rel.join();
        }
    }
    CHECK(cec_pipeline_drain(pl) == CEC_OK, "drain");
    for (size_t s = 0; s < depth; ++s)
        if (pend[s].used) collect(s);
    standin_log(false);

    // The copy geometry, from the log: per batch, on the slot's one stream, the uploads, the
    // compute, the downloads and the event, in that order and with nothing else between; the
    // uploads' destinations are exactly the L bytes of every data chunk at stride cs, the parity
    // downloads' sources exactly those of the parity chunks, and no two copies overlap.
    const std::vector<StandinOp> ops = standin_ops();
    size_t batches_seen = 0;
    for (size_t s = 0; s < depth; ++s) {
        const unsigned sn = standin_stream_number(streams[s]);
        std::vector<StandinOp> mine;
        for (const StandinOp& o : ops)
            if (o.stream == sn) mine.push_back(o);
        size_t at = 0;
        uint64_t pos = 0;
        for (size_t b : slot_batches[s]) {
            const size_t n = nb[b], ncopy_up = cs == L ? 1 : d, ncopy_down = cs == L ? 1 : p;
            CHECK(at + ncopy_up + 1 + ncopy_down + 2 <= mine.size(), "batch %zu: operations missing", b);
            std::vector<std::pair<size_t, size_t>> up, down, host_out;
            int dbuf = -1;
            for (size_t j = 0; j < ncopy_up; ++j, ++at) {
                const StandinOp& o = mine[at];
                CHECK(o.type == StandinOp::Copy && o.kind == hipMemcpyHostToDevice && o.pos == ++pos,
                      "batch %zu: operation %zu is not its upload %zu", b, at, j);
                if (j == 0) dbuf = o.dst_alloc;
                CHECK(o.dst_alloc == dbuf && o.rows == n && o.dpitch == t * cs,
                      "batch %zu upload %zu: rows %zu pitch %zu", b, j, o.rows, o.dpitch);
                for (size_t k = 0; k < o.rows; ++k) up.emplace_back(o.dst_off + k * o.dpitch, o.width);
            }
            CHECK(mine[at].type == StandinOp::Launch && !std::strcmp(mine[at].label, "encode_hash") &&
                      mine[at].pos == ++pos, "batch %zu: the compute does not follow the uploads", b);
            ++at;
            for (size_t i = 0; i < ncopy_down; ++i, ++at) {
                const StandinOp& o = mine[at];
                CHECK(o.type == StandinOp::Copy && o.kind == hipMemcpyDeviceToHost && o.pos == ++pos &&
                          o.src_alloc == dbuf && o.rows == n && o.spitch == t * cs,
                      "batch %zu: operation %zu is not its parity download %zu", b, at, i);
                for (size_t k = 0; k < o.rows; ++k) {
                    down.emplace_back(o.src_off + k * o.spitch, o.width);
                    host_out.emplace_back(o.dst_off + k * o.dpitch, o.width);
                }
            }
            CHECK(mine[at].type == StandinOp::Copy && mine[at].kind == hipMemcpyDeviceToHost &&
                      mine[at].rows == 1 && mine[at].width == n * t * 32 && mine[at].src_off == 0 &&
                      mine[at].src_alloc != dbuf && mine[at].pos == ++pos,
                  "batch %zu: the digest download", b);
            ++at;
            CHECK(mine[at].type == StandinOp::EventRecord && mine[at].pos == pos,
                  "batch %zu: the event is not recorded right behind the downloads", b);
            ++at;
            // expected ranges, merged where chunks touch (cs == L: whole rows)
            auto canon = [](std::vector<std::pair<size_t, size_t>> v, const char* what, size_t b) {
                std::sort(v.begin(), v.end());
                std::vector<std::pair<size_t, size_t>> out;
                for (auto& x : v) {
                    CHECK(out.empty() || out.back().first + out.back().second <= x.first,
                          "batch %zu: two %s copies overlap at byte %zu", b, what, x.first);
                    if (!out.empty() && out.back().first + out.back().second == x.first)
                        out.back().second += x.second;
                    else
                        out.push_back(x);
                }
                return out;
            };
            std::vector<std::pair<size_t, size_t>> want_up, want_down;
            for (size_t k = 0; k < n; ++k) {
                for (size_t j = 0; j < d; ++j) want_up.emplace_back(k * t * cs + j * cs, L);
                for (size_t i = 0; i < p; ++i) want_down.emplace_back(k * t * cs + (d + i) * cs, L);
            }
            CHECK(canon(up, "upload", b) == canon(want_up, "expected upload", b),
                  "batch %zu: the uploads do not cover exactly the data chunks", b);
            CHECK(canon(down, "download", b) == canon(want_down, "expected download", b),
                  "batch %zu: the downloads do not read exactly the parity chunks", b);
            const auto out = canon(host_out, "parity output", b);
            CHECK(out.size() == 1 && out[0].second == n * p * L,
                  "batch %zu: the parity output is not one dense [n][p][L] range", b);
            ++batches_seen;
        }
        CHECK(at == mine.size(), "stream of slot %zu has %zu operations no batch accounts for", s,
              mine.size() - at);
    }
    CHECK(batches_seen == B, "the log shows %zu batches, not %zu", batches_seen, B);
    check_slots_used();
    cec_pipeline_free(pl);
    finish();
}

// ------------------------------------------------------------------------------------------
// b. Read pipeline
// ------------------------------------------------------------------------------------------
// Submits case c on `slot` (acquired by the caller: ch / pr / ex are the slot's arrays, ch null
// for an external pipeline) and returns the buffers that must live until the wait.
struct ReadBatch {
    ReadCase c;
    unsigned mode = 0;
    BufP in, out;
    bool used = false;
};
void fill_slot(const ReadCase& c, uint8_t* ch, uint8_t* pr, uint8_t* ex) {
    std::memcpy(ch, c.chunks.data(), c.chunks.size());
    std::memcpy(pr, c.present.data(), c.present.size());
    std::memcpy(ex, c.expected.data(), c.expected.size());
}
size_t mode_out(unsigned mode, size_t d, size_t t) {
    return (mode & CEC_READ_VERIFY_ONLY) ? 0 : (mode & CEC_READ_RESILVER) ? t : d;
}
void check_read_slot(cec_read_pipeline* pl, size_t slot, ReadBatch& q, const Fix& f) {
    const uint8_t *data = nullptr, *ver = nullptr;
    const int* status = nullptr;
    size_t got = 0;
    CHECK(cec_read_pipeline_wait(pl, slot, &data, &ver, &status, &got) == CEC_OK, "read wait: %s",
          cec_pipeline_last_error());
    CHECK(cec_read_pipeline_query(pl, slot) == 1 && got == q.c.n, "read wait: %zu parts", got);
    check_verified(q.c, ver, "read pipeline");
    const size_t W = mode_out(q.mode, f.d, f.t);
    if (W) {
        std::vector<const uint8_t*> ptrs(q.c.n * W, nullptr);
        CHECK(cec_read_pipeline_data_chunks(pl, slot, ptrs.data(), ptrs.size()) == CEC_OK, "data_chunks");
        check_chunks(q.c, f, status, ptrs.data(), W, "read pipeline");
        if (!(q.mode & (CEC_READ_REBUILT_ONLY | CEC_READ_RESILVER)))  // plain read: dense [n][d][L]
            for (size_t k = 0; k < q.c.n; ++k)
                if (status[k] == CEC_OK)
                    CHECK(std::memcmp(data + k * f.d * f.L, f.data.data() + q.c.part[k] * f.d * f.L,
                                      f.d * f.L) == 0, "result mismatch: read data of part %zu", k);
    } else {
        for (size_t k = 0; k < q.c.n; ++k) CHECK(status[k] == CEC_OK, "verify status");
    }
    for (Buf* x : {q.in.get(), q.out.get()})
        if (x) x->check("read batch buffer");
    q = ReadBatch{};
}

void scenario_read(size_t d, size_t p, size_t L, size_t P, size_t depth, uint64_t seed) {
    begin("b read RS(%zu,%zu) L=%zu P=%zu depth=%zu seed=%llu", d, p, L, P, depth,
          (unsigned long long)seed);
    set_schedule(seed, g_mutant);
    const size_t t = d + p;
    Codec codec(d, p);
    cec_read_pipeline* pl = nullptr;
    CHECK(cec_read_pipeline_new_ex(codec.c, L, P, depth, 0u, &pl) == CEC_OK, "read pipeline: %s",
          cec_pipeline_last_error());
    std::vector<hipStream_t> streams = standin_streams();
    CHECK(streams.size() == depth, "one stream per slot");
    if (depth >= 2) {
        // the last slot as the scheduler makes its AHEAD slots: a stream of the greatest priority
        // in place of the plain one (which is destroyed idle)
        CHECK(cec::read_pipeline_priority_slot(pl, depth - 1) == CEC_OK, "priority slot: %s",
              cec_pipeline_last_error());
        const std::vector<hipStream_t> now = standin_streams();
        CHECK(now.size() == depth && now.back() != streams.back() &&
                  standin_calls("hipStreamCreateWithPriority") == 1, "the slot's stream was replaced");
        streams = now;
    }
    Rng r(seed);
    const Fix f = make_fix(d, p, L, 2 * P, seed);
    const unsigned modes[4] = {0u, CEC_READ_REBUILT_ONLY, CEC_READ_RESILVER, CEC_READ_VERIFY_ONLY};
    std::vector<ReadBatch> pend(depth);
    const size_t B = std::max<size_t>(8, 3 * depth + 2);
    for (size_t b = 0; b < B; ++b) {
        size_t slot = 0;
        uint8_t *ch = nullptr, *pr = nullptr, *ex = nullptr;
        if (b % 2)
            CHECK(cec_read_pipeline_acquire(pl, &slot, &ch, &pr, &ex) == CEC_OK, "acquire");
        else
            CHECK(cec_read_pipeline_acquire_idle(pl, &slot, &ch, &pr, &ex) == CEC_OK, "acquire_idle");
        if (pend[slot].used) check_read_slot(pl, slot, pend[slot], f);
        ReadBatch& q = pend[slot];
        const size_t n = b % 3 == 2 ? 1 + r.below(P) : P;
        std::vector<size_t> parts(n);
        std::vector<int> kinds(n);
        for (size_t k = 0; k < n; ++k) {
            parts[k] = r.below(f.n);
            kinds[k] = k < 4 ? int((k + b) % 4) : int(r.below(4));  // every kind in every batch
        }
        q.c = make_read(f, parts, kinds, r);
        q.mode = modes[b % 4];
        q.used = true;
        const bool packed = (b / 4) % 2 == 1;
        const size_t W = mode_out(q.mode, d, t);
        cec_read_submit a{};
        a.n_parts = n;
        a.flags = q.mode;
        // the slot's own output holds d chunks per part: resilver brings its own
        if (W == t || (W && b % 2)) {
            q.out = buf(n * W * L, true);
            a.data_out = q.out->p();
        }
        const bool hold = b == 0;
        if (hold) standin_hold(streams[slot]);
        if (packed) {
            size_t m = 0;
            for (uint8_t fl : q.c.present) m += fl ? 1 : 0;
            q.in = buf(std::max<size_t>(m, 1) * L, true);
            size_t at = 0;
            for (size_t x = 0; x < n * t; ++x)
                if (q.c.present[x]) std::memcpy(q.in->p() + (at++) * L, q.c.chunks.data() + x * L, L);
            a.chunks = q.in->p();
            a.present = q.c.present.data();
            a.expected = q.c.expected.data();
            a.flags |= CEC_SUBMIT_PACKED;
        } else {
            fill_slot(q.c, ch, pr, ex);
        }
        CHECK(cec_read_pipeline_submit_ex(pl, slot, &a) == CEC_OK, "read submit: %s",
              cec_pipeline_last_error());
        if (hold) {
            sleep_us(300);
            CHECK(cec_read_pipeline_query(pl, slot) == 0, "query is 0 while the slot's stream is held");
            std::thread rel([&] { sleep_us(1500); standin_release(streams[slot]); });
            check_read_slot(pl, slot, q, f);
            rel.join();
        }
    }
    CHECK(cec_read_pipeline_drain(pl) == CEC_OK, "drain");
    for (size_t s = 0; s < depth; ++s)
        if (pend[s].used) check_read_slot(pl, s, pend[s], f);
    check_slots_used();
    cec_read_pipeline_free(pl);
    finish();
}

// CEC_READ_CARRY: stash, carry_ids, the retry's submit_carried, carry_release, entries given back
// by the slot's next submit, a reservation that runs out, and the reuse of an entry whose
// consuming move is still queued on another slot's held stream (what hipStreamWaitEvent is for).
void scenario_carry(size_t d, size_t p, size_t L, size_t P, size_t depth, uint64_t seed) {
    begin("b carry RS(%zu,%zu) L=%zu P=%zu depth=%zu seed=%llu", d, p, L, P, depth,
          (unsigned long long)seed);
    set_schedule(seed, g_mutant);
    Codec codec(d, p);
    cec_read_pipeline* pl = nullptr;
    CHECK(cec_read_pipeline_new_ex(codec.c, L, P, depth, CEC_READ_CARRY, &pl) == CEC_OK,
          "read pipeline: %s", cec_pipeline_last_error());
    const std::vector<hipStream_t> streams = standin_streams();
    Rng r(seed);
    const Fix f = make_fix(d, p, L, 3 * P, seed);
    const size_t cap = P * (depth + 1);  // carry_batch = P for P <= 8
    struct Held {
        int32_t id;
        size_t part;
    };
    std::vector<Held> held;
    // A batch of n parts of the given kinds on the next slot; returns the slot.
    auto submit = [&](ReadBatch& q, const std::vector<size_t>& parts, const std::vector<int>& kinds,
                      const std::vector<int32_t>* ids, const std::vector<size_t>& retries,
                      bool hold_slot) {
        size_t slot = 0;
        uint8_t *ch = nullptr, *pr = nullptr, *ex = nullptr;
        CHECK(cec_read_pipeline_acquire(pl, &slot, &ch, &pr, &ex) == CEC_OK, "acquire");
        q.c = make_read(f, parts, kinds, r);
        for (size_t k : retries) retry_of_kind3(q.c, k, f);
        q.mode = 0;
        q.used = true;
        fill_slot(q.c, ch, pr, ex);
        if (hold_slot) standin_hold(streams[slot]);
        const int st = ids ? cec_read_pipeline_submit_carried(pl, slot, parts.size(), ids->data())
                           : cec_read_pipeline_submit(pl, slot, parts.size());
        CHECK(st == CEC_OK, "carry submit: %s", cec_pipeline_last_error());
        return slot;
    };
    auto claim = [&](size_t slot, const ReadBatch& q, std::vector<int32_t>& ids) {
        ids.assign(q.c.n, -2);
        CHECK(cec_read_pipeline_carry_ids(pl, slot, ids.data(), ids.size()) == CEC_OK, "carry_ids");
    };
    const std::vector<int> all_fail(P, 3);
    std::vector<size_t> parts(P);
    std::vector<int32_t> ids;

    // 1. one part fails, its verified chunks are kept; the retry takes them from the pool
    {
        ReadBatch q;
        for (size_t k = 0; k < P; ++k) parts[k] = k;
        std::vector<int> kinds(P, 0);
        kinds[1] = 3;
        kinds[P - 1] = 2;
        const size_t slot = submit(q, parts, kinds, nullptr, {}, false);
        ReadCase c = q.c;
        check_read_slot(pl, slot, q, f);
        q.c = c;
        claim(slot, q, ids);
        for (size_t k = 0; k < P; ++k)
            CHECK((ids[k] >= 0) == (k == 1), "carry id of part %zu is %d", k, ids[k]);
        CHECK(cec_read_pipeline_carry_held(pl) == 1, "one entry held");
        // the retry sits at another position of its batch, among fresh parts
        ReadBatch q2;
        std::vector<size_t> parts2(P);
        std::vector<int32_t> ids2(P, -1);
        for (size_t k = 0; k < P; ++k) parts2[k] = P + k;
        parts2[P - 1] = 1;
        ids2[P - 1] = ids[1];
        std::vector<int> kinds2(P, 1);
        kinds2[P - 1] = 3;
        // an id given for a part it was not kept for is refused, and stays held
        {
            std::vector<int32_t> wrong(P, -1);
            wrong[0] = ids[1];
            size_t slot2 = 0;
            uint8_t *ch = nullptr, *pr = nullptr, *ex = nullptr;
            CHECK(cec_read_pipeline_acquire(pl, &slot2, &ch, &pr, &ex) == CEC_OK, "acquire");
            ReadCase w = make_read(f, parts2, kinds2, r);
            fill_slot(w, ch, pr, ex);
            CHECK(cec_read_pipeline_submit_carried(pl, slot2, P, wrong.data()) ==
                      CEC_ERR_INVALID_ARGUMENT, "a carry id of another part is refused");
            CHECK(cec_read_pipeline_carry_held(pl) == 1, "the refused id stays held");
        }
        const size_t slot2 = submit(q2, parts2, kinds2, &ids2, {P - 1}, false);
        check_read_slot(pl, slot2, q2, f);
        CHECK(cec_read_pipeline_carry_held(pl) == 0, "the retry used the entry");
        CHECK(cec_read_pipeline_carry_release(pl, ids[1]) == CEC_ERR_INVALID_ARGUMENT,
              "an id is used once");
    }
    // 2. entries nobody claims go back with the slot's next submit: depth + 2 failing batches
    //    never claimed, and the pool is whole afterwards (3. needs every entry)
    for (size_t b = 0; b < depth + 2; ++b) {
        ReadBatch q;
        for (size_t k = 0; k < P; ++k) parts[k] = r.below(f.n);
        const size_t slot = submit(q, parts, all_fail, nullptr, {}, false);
        check_read_slot(pl, slot, q, f);
        CHECK(cec_read_pipeline_carry_held(pl) == 0, "unclaimed entries are not held");
    }
    // 3. every part of depth + 1 batches fails and is claimed: the pool is full, the next batch's
    //    reservation runs out (ids -1, the parts still TooFewShardsPresent)
    for (size_t b = 0; b < depth + 2; ++b) {
        ReadBatch q;
        for (size_t k = 0; k < P; ++k) parts[k] = (b * P + k) % f.n;
        const size_t slot = submit(q, parts, all_fail, nullptr, {}, false);
        ReadCase c = q.c;
        check_read_slot(pl, slot, q, f);
        q.c = c;
        claim(slot, q, ids);
        for (size_t k = 0; k < P; ++k) {
            CHECK((ids[k] >= 0) == (b <= depth), "batch %zu part %zu: carry id %d (pool of %zu)", b, k,
                  ids[k], cap);
            if (ids[k] >= 0) held.push_back({ids[k], parts[k]});
        }
    }
    CHECK(held.size() == cap && cec_read_pipeline_carry_held(pl) == cap, "the pool is full");
    // 4. (depth >= 2) P entries go back, then the retry of held entry X is queued on slot B whose
    //    stream is HELD: its move (pool -> batch) has not run, X is back in the free list behind
    //    the P entries B's own stash reserved.  Slot A's batch fails every part: its stash reserves
    //    X, and must wait (hipStreamWaitEvent on X's event, recorded on B behind the move) before it
    //    overwrites X.  Without that wait B's retry decodes another part's chunks.
    if (depth >= 2) {
        const Held x = held.back();
        held.pop_back();
        for (size_t k = 0; k < P; ++k) {
            CHECK(cec_read_pipeline_carry_release(pl, held.back().id) == CEC_OK, "carry_release");
            held.pop_back();
        }
        ReadBatch qb, qa;
        std::vector<size_t> pb(P);
        std::vector<int> kb(P, 0);
        std::vector<int32_t> ib(P, -1);
        for (size_t k = 0; k < P; ++k) pb[k] = r.below(f.n);
        pb[0] = x.part;
        kb[0] = 3;
        ib[0] = x.id;
        const size_t sb = submit(qb, pb, kb, &ib, {0}, true);
        for (size_t k = 0; k < P; ++k) parts[k] = (x.part + 1 + k) % f.n;
        const size_t sa = submit(qa, parts, all_fail, nullptr, {}, false);
        CHECK(sa != sb, "two slots");
        sleep_us(8000);
        const bool a_waited = cec_read_pipeline_query(pl, sa) == 0;
        standin_release(streams[sb]);
        check_read_slot(pl, sb, qb, f);
        CHECK(a_waited, "slot A's batch completed with the move on slot B's held stream still queued");
        ReadCase c = qa.c;
        check_read_slot(pl, sa, qa, f);
        qa.c = c;
        claim(sa, qa, ids);
        CHECK(ids[0] == x.id, "slot A's first failing part got the entry the retry freed");
        for (size_t k = 1; k < P; ++k) CHECK(ids[k] == -1, "one entry was free");
        held.push_back({ids[0], parts[0]});
    }
    for (const Held& h : held)
        CHECK(cec_read_pipeline_carry_release(pl, h.id) == CEC_OK, "carry_release");
    CHECK(cec_read_pipeline_carry_held(pl) == 0, "everything released");
    // the pool serves again
    {
        ReadBatch q;
        for (size_t k = 0; k < P; ++k) parts[k] = k;
        const size_t slot = submit(q, parts, all_fail, nullptr, {}, false);
        ReadCase c = q.c;
        check_read_slot(pl, slot, q, f);
        q.c = c;
        claim(slot, q, ids);
        for (size_t k = 0; k < P; ++k) {
            CHECK(ids[k] >= 0, "the released pool serves again");
            CHECK(cec_read_pipeline_carry_release(pl, ids[k]) == CEC_OK, "carry_release");
        }
    }
    check_slots_used();
    cec_read_pipeline_free(pl);
    finish();
}

// ------------------------------------------------------------------------------------------
// c. Scheduler
// ------------------------------------------------------------------------------------------
struct Multi {
    cec_multi* m = nullptr;
    Multi(const Codec& c, size_t L, size_t P, size_t depth, const std::vector<int>& devices) {
        standin_set_devices(1 + *std::max_element(devices.begin(), devices.end()));
        CHECK(cec_multi_new_ex(c.c, L, P, depth, devices.data(), devices.size(),
                               CEC_MULTI_WRITE | CEC_MULTI_READ, &m) == CEC_OK,
              "cec_multi_new_ex: %s", cec_multi_last_error());
    }
    ~Multi() {
        if (m) cec_multi_free(m);
    }
    void free() {
        cec_multi_free(m);
        m = nullptr;
    }
};

struct WriteJob {
    size_t first = 0, n = 0;
    BufP in, par, dig;
    uint64_t id = 0;
    void submit(cec_multi* m, const Fix& f, size_t first_part, size_t n_parts, bool pin) {
        first = first_part;
        n = n_parts;
        in = buf(n * f.d * f.L, pin);
        par = buf(n * f.p * f.L, pin);
        dig = buf(n * f.t * 32, pin);
        std::memcpy(in->p(), f.data.data() + first * f.d * f.L, n * f.d * f.L);
        CHECK(cec_multi_encode_hash(m, in->p(), n, par->p(), dig->p(), &id) == CEC_OK,
              "cec_multi_encode_hash");
    }
    void check(const Fix& f) {
        CHECK(std::memcmp(par->p(), f.parity.data() + first * f.p * f.L, n * f.p * f.L) == 0,
              "result mismatch: scheduler parity (job of %zu parts)", n);
        CHECK(std::memcmp(dig->p(), f.dig.data() + first * f.t * 32, n * f.t * 32) == 0,
              "result mismatch: scheduler digests (job of %zu parts)", n);
        in->check("job data");
        par->check("job parity");
        dig->check("job digests");
    }
};

enum class RKind { Read, Rebuilt, Resilver, Verify };
struct ReadJob {
    RKind kind = RKind::Read;
    ReadCase c;
    BufP in, out, ver;
    std::vector<int> status;
    std::vector<const uint8_t*> ptrs;
    std::vector<int32_t> carry_out;
    uint64_t id = 0;
    size_t W = 0;
    int submit(cec_multi* m, const Fix& f, ReadCase rc, RKind k, bool pin, unsigned flags = 0,
               const int32_t* carry_in = nullptr, bool want_carry = false) {
        c = std::move(rc);
        kind = k;
        W = k == RKind::Verify ? 0 : k == RKind::Resilver ? f.t : f.d;
        const size_t n = c.n;
        in = buf(std::max<size_t>(c.chunks.size(), 1), pin);
        if (!c.chunks.empty()) std::memcpy(in->p(), c.chunks.data(), c.chunks.size());
        out = buf(std::max<size_t>(n * W * f.L, 1), pin);
        ver = buf(std::max<size_t>(n * f.t, 1), false);
        status.assign(std::max<size_t>(n, 1), -7);
        ptrs.assign(std::max<size_t>(n * W, 1), nullptr);
        if (want_carry) carry_out.assign(std::max<size_t>(n, 1), -2);
        switch (k) {
            case RKind::Verify:
                return cec_multi_verify(m, in->p(), c.present.data(), c.expected.data(), n, ver->p(), &id);
            case RKind::Resilver:
                return cec_multi_resilver(m, in->p(), c.present.data(), c.expected.data(), n, out->p(),
                                          ver->p(), status.data(), ptrs.data(), &id);
            default:
                return cec_multi_read_carry(
                    m, in->p(), c.present.data(), c.expected.data(), n, out->p(), ver->p(),
                    status.data(), ptrs.data(), flags | (k == RKind::Rebuilt ? CEC_READ_REBUILT_ONLY : 0u),
                    carry_in, want_carry ? carry_out.data() : nullptr, &id);
        }
    }
    void check(const Fix& f) {
        check_verified(c, ver->p(), "scheduler");
        if (kind == RKind::Read) {  // every result at its part's own position
            std::vector<const uint8_t*> at(c.n * f.d);
            for (size_t x = 0; x < at.size(); ++x) at[x] = out->p() + x * f.L;
            check_chunks(c, f, status.data(), at.data(), f.d, "scheduler read");
        } else if (W) {
            check_chunks(c, f, status.data(), ptrs.data(), W, "scheduler read");
        }
        in->check("job chunks");
        out->check("job output");
        ver->check("job verified");
    }
};

ReadCase random_case(const Fix& f, size_t n, Rng& r, int only_kind = -1) {
    std::vector<size_t> parts(n);
    std::vector<int> kinds(n);
    for (size_t k = 0; k < n; ++k) {
        parts[k] = r.below(f.n);
        kinds[k] = only_kind >= 0 ? only_kind : int(r.below(4));
    }
    return make_read(f, parts, kinds, r);
}

void scenario_multi(size_t d, size_t p, size_t L, size_t P, size_t depth,
                    const std::vector<int>& devices, uint64_t seed) {
    const size_t G = devices.size();
    begin("c scheduler RS(%zu,%zu) L=%zu P=%zu depth=%zu shards=%zu%s seed=%llu", d, p, L, P, depth, G,
          G == 2 ? (devices[1] ? " [0,1]" : " [0,0]") : "", (unsigned long long)seed);
    set_schedule(seed, g_mutant);
    Codec codec(d, p);
    Multi mu(codec, L, P, depth, devices);
    cec_multi* m = mu.m;
    CHECK(cec_multi_shards(m) == G, "shards");
    Rng r(seed);
    const size_t big = P * depth * G + 1;
    const Fix f = make_fix(d, p, L, big, seed);
    const size_t sizes[4] = {0, 1, G - 1, big};

    // pageable jobs go through the shard's pinned staging, sized by the job's mode: a resilver
    // (d+p chunks out per part) queued behind a read (d chunks) whose batches are still in flight
    // must not replace the staging those batches copy into and are finished from
    {
        standin_hold_all();
        ReadJob rd, rs;
        // the read leaves one depth slot free (depth >= 2): the resilver takes it at once, with the
        // read's batches certainly still in flight on the others
        CHECK(rd.submit(m, f, random_case(f, P * std::max<size_t>(depth - 1, 1) * G, r), RKind::Read,
                        false) == CEC_OK, "read");
        CHECK(rs.submit(m, f, random_case(f, P * G, r), RKind::Resilver, false) == CEC_OK, "resilver");
        sleep_us(3000);
        standin_release_all();
        CHECK(cec_multi_wait(m, rs.id) == CEC_OK && cec_multi_wait(m, rd.id) == CEC_OK, "waits");
        rd.check(f);
        rs.check(f);
        check_clean("after a resilver behind a read in flight, both through staging");
    }
    // jobs of every size and kind interleaved, pinned and pageable, waited for in another order
    {
        std::vector<std::unique_ptr<WriteJob>> wj;
        std::vector<std::unique_ptr<ReadJob>> rj;
        const RKind kinds[4] = {RKind::Read, RKind::Rebuilt, RKind::Resilver, RKind::Verify};
        size_t q = 0;
        for (size_t n : sizes) {
            wj.push_back(std::make_unique<WriteJob>());
            wj.back()->submit(m, f, n == big ? 0 : r.below(big - n + 1), n, (q++ + seed) % 2 == 0);
            for (RKind k : kinds) {
                rj.push_back(std::make_unique<ReadJob>());
                CHECK(rj.back()->submit(m, f, random_case(f, n, r), k, (q++ + seed) % 2 == 0) == CEC_OK,
                      "read job submit");
            }
        }
        // poll one job, then wait in reverse order
        CHECK(cec_multi_query(m, wj[0]->id) == 1, "a job of no parts is complete at once");
        while (cec_multi_query(m, wj[3]->id) == 0) sleep_us(100);
        for (size_t i = rj.size(); i-- > 0;) {
            CHECK(cec_multi_wait(m, rj[i]->id) == CEC_OK, "read job wait: %s", cec_multi_last_error());
            CHECK(cec_multi_query(m, rj[i]->id) == CEC_ERR_INVALID_ARGUMENT, "a job is waited for once");
            rj[i]->check(f);
        }
        for (size_t i = wj.size(); i-- > 0;) {
            CHECK(cec_multi_query(m, wj[i]->id) >= 0, "query");
            CHECK(cec_multi_wait(m, wj[i]->id) == CEC_OK, "write job wait: %s", cec_multi_last_error());
            wj[i]->check(f);
        }
    }
    // an AHEAD read queued behind held work: three AHEAD batches per shard stay in flight
    {
        // the window fills every depth slot of every shard and stays there; the AHEAD job, queued
        // behind it, takes the AHEAD slots (three batches per shard, all in flight at once); the
        // write job behind both waits for the read batches
        auto uploaded = [&] {
            uint64_t sum = 0;
            cec_multi_stats st{};
            for (size_t g = 0; g < G; ++g) {
                CHECK(cec_multi_shard_stats(m, g, &st) == CEC_OK, "stats");
                sum += st.chunks_uploaded;
            }
            return sum;
        };
        const uint64_t up0 = uploaded();
        standin_hold_all();
        ReadJob window, retry;
        WriteJob w;
        CHECK(window.submit(m, f, random_case(f, P * depth * G, r), RKind::Rebuilt, true) == CEC_OK,
              "window");
        CHECK(retry.submit(m, f, random_case(f, 3 * P * G, r), RKind::Read, true, CEC_MULTI_AHEAD) ==
                  CEC_OK, "AHEAD job");
        w.submit(m, f, 0, big, true);
        // until both read jobs' batches are all queued (the shards count the chunks they send)
        uint64_t want = up0;
        for (uint8_t fl : window.c.present) want += fl ? 1 : 0;
        for (uint8_t fl : retry.c.present) want += fl ? 1 : 0;
        for (int spin = 0; uploaded() < want && spin < 50000; ++spin) sleep_us(100);
        CHECK(uploaded() == want, "the held read jobs were not queued within 5 s");
        CHECK(cec_multi_query(m, retry.id) == 0 && cec_multi_query(m, w.id) == 0,
              "nothing completes on held streams");
        standin_release_all();
        CHECK(cec_multi_wait(m, retry.id) == CEC_OK, "AHEAD wait: %s", cec_multi_last_error());
        retry.check(f);
        CHECK(cec_multi_wait(m, window.id) == CEC_OK && cec_multi_wait(m, w.id) == CEC_OK, "waits");
        window.check(f);
        w.check(f);
    }
    // a carry round trip: the failed parts' ids name the shard that holds their chunks, and the
    // retry job sends each part there wherever it sits in the job
    {
        const size_t n = 2 * G + 3;
        std::vector<size_t> parts(n);
        std::vector<int> kinds(n);
        for (size_t k = 0; k < n; ++k) {
            parts[k] = r.below(f.n);
            kinds[k] = k % 2 ? 3 : int(r.below(3));
        }
        ReadJob first;
        CHECK(first.submit(m, f, make_read(f, parts, kinds, r), RKind::Rebuilt, seed % 2 == 0, 0,
                           nullptr, true) == CEC_OK, "carry job");
        CHECK(cec_multi_wait(m, first.id) == CEC_OK, "carry job wait: %s", cec_multi_last_error());
        first.check(f);
        std::vector<size_t> parts2;
        std::vector<int> kinds2;
        std::vector<int32_t> in2;
        std::vector<size_t> retries;
        uint64_t held = 0;
        int32_t spare = -1;  // one id is not used again but given back
        for (size_t k = n; k-- > 0;) {  // reversed: the contiguous split would misroute them
            const int32_t id = first.carry_out[k];
            CHECK((id >= 0) == (kinds[k] == 3), "carry_out of part %zu is %d", k, id);
            if (id < 0) continue;
            CHECK(size_t(id >> 20) < G, "carry id %d names no shard", id);
            ++held;
            if (spare < 0) {
                spare = id;
                continue;
            }
            retries.push_back(parts2.size());
            parts2.push_back(parts[k]);
            kinds2.push_back(3);
            in2.push_back(id);
            parts2.push_back(r.below(f.n));  // a fresh part between the retries
            kinds2.push_back(1);
            in2.push_back(-1);
        }
        cec_multi_stats st{};
        uint64_t sum = 0, carried0 = 0;
        for (size_t g = 0; g < G; ++g) {
            CHECK(cec_multi_shard_stats(m, g, &st) == CEC_OK, "stats");
            sum += st.carry_held;
            carried0 += st.chunks_carried;
        }
        CHECK(sum == held, "%llu entries held, %llu ids given", (unsigned long long)sum,
              (unsigned long long)held);
        ReadCase c2 = make_read(f, parts2, kinds2, r);
        for (size_t k : retries) retry_of_kind3(c2, k, f);
        // a carry id of no shard is refused at submit
        {
            std::vector<int32_t> bad = in2;
            bad[0] = int32_t(G << 20) | 1;
            ReadJob refused;
            CHECK(refused.submit(m, f, c2, RKind::Read, false, 0, bad.data()) == CEC_ERR_INVALID_ARGUMENT,
                  "a carry id of no shard is refused");
        }
        CHECK(held >= 2 && !retries.empty(), "the carry job has too few failed parts");
        ReadJob second;
        CHECK(second.submit(m, f, c2, RKind::Read, seed % 2 == 1, CEC_MULTI_AHEAD, in2.data()) == CEC_OK,
              "retry job");
        CHECK(cec_multi_wait(m, second.id) == CEC_OK, "retry job wait: %s", cec_multi_last_error());
        second.check(f);
        CHECK(cec_multi_carry_release(m, spare) == CEC_OK, "cec_multi_carry_release");
        uint64_t carried = 0;
        for (int spin = 0; spin < 20000; ++spin) {
            sum = carried = 0;
            for (size_t g = 0; g < G; ++g) {
                CHECK(cec_multi_shard_stats(m, g, &st) == CEC_OK, "stats");
                sum += st.carry_held;
                carried += st.chunks_carried;
            }
            if (sum == 0) break;
            sleep_us(100);
        }
        CHECK(sum == 0, "entries still held after the retry and the release");
        CHECK(carried - carried0 == (held - 1) * (d - 1), "%llu chunks came from the carry pool, not %llu",
              (unsigned long long)(carried - carried0), (unsigned long long)((held - 1) * (d - 1)));
    }
    check_slots_used();
    mu.free();
    finish();
}

// ------------------------------------------------------------------------------------------
// d. Lifecycle
// ------------------------------------------------------------------------------------------
void lifecycle_cycles(const std::vector<int>& devices, size_t cycles, uint64_t seed) {
    begin("d %zu create / damaged read / free cycles on %zu shards seed=%llu", cycles, devices.size(),
          (unsigned long long)seed);
    const size_t d = 3, p = 2, L = 64, P = 4;
    Codec codec(d, p);
    Rng r(seed);
    const Fix f = make_fix(d, p, L, 4 * P, seed);
    for (size_t c = 0; c < cycles; ++c) {
        set_schedule(seed * 1000 + c, g_mutant);
        {
            Multi mu(codec, L, P, 1 + c % 2, devices);
            ReadJob j;
            CHECK(j.submit(mu.m, f, random_case(f, 1 + r.below(3 * P), r), c % 2 ? RKind::Read : RKind::Rebuilt,
                           c % 3 == 0) == CEC_OK, "read job");
            CHECK(cec_multi_wait(mu.m, j.id) == CEC_OK, "wait: %s", cec_multi_last_error());
            j.check(f);
            mu.free();
        }
        check_clean("in a cycle");
        if (c % 8 == 7) {
            finish();
            standin_reset();
        }
    }
    finish();
}

void scenario_lifecycle(uint64_t seed) {
    const size_t d = 3, p = 2, L = 64, P = 4, depth = 2;
    const std::vector<std::vector<int>> layouts = {{0}, {0, 0}, {0, 1}};
    for (const auto& devices : layouts) {
        const size_t G = devices.size();
        begin("d lifecycle on %zu shards seed=%llu", G, (unsigned long long)seed);
        set_schedule(seed, g_mutant);
        Codec codec(d, p);
        Rng r(seed);
        const Fix f = make_fix(d, p, L, P * depth * G + 1, seed);
        {  // new and free with no job
            Multi mu(codec, L, P, depth, devices);
        }
        check_clean("after new + free");
        {  // jobs finished but never waited for
            Multi mu(codec, L, P, depth, devices);
            WriteJob w;
            ReadJob j;
            w.submit(mu.m, f, 0, f.n, false);
            CHECK(j.submit(mu.m, f, random_case(f, f.n, r), RKind::Resilver, true) == CEC_OK, "job");
            while (cec_multi_query(mu.m, w.id) == 0 || cec_multi_query(mu.m, j.id) == 0) sleep_us(100);
            mu.free();
            w.check(f);
            j.check(f);
        }
        check_clean("after a free with unwaited jobs");
        {  // free while every stream is held; another thread releases them a moment later: the
           // destructors must wait for the queued work, not destroy under it
            Multi mu(codec, L, P, depth, devices);
            WriteJob w;
            ReadJob j;
            standin_hold_all();
            w.submit(mu.m, f, 0, f.n, true);
            CHECK(j.submit(mu.m, f, random_case(f, f.n, r), RKind::Read, true) == CEC_OK, "job");
            std::thread rel([] { sleep_us(3000); standin_release_all(); });
            mu.free();
            rel.join();
            w.check(f);  // the jobs ran to their end before the scheduler went
            j.check(f);
        }
        finish();
    }
    lifecycle_cycles({0}, 40, seed);
    lifecycle_cycles({0, 1}, 40, seed);
    lifecycle_cycles({0, 0}, 16, seed);

    // two schedulers driven from two host threads at once
    {
        begin("d two schedulers, two host threads seed=%llu", (unsigned long long)seed);
        set_schedule(seed, g_mutant);
        standin_set_devices(2);
        Codec codec(d, p);
        const Fix f = make_fix(d, p, L, 3 * P, seed);
        auto drive = [&](int which) {
            Rng r(seed * 2 + uint64_t(which));
            const std::vector<int> devices = which ? std::vector<int>{1, 0} : std::vector<int>{0, 1};
            cec_multi* m = nullptr;
            CHECK(cec_multi_new(codec.c, L, P, depth, devices.data(), 2, &m) == CEC_OK, "cec_multi_new");
            for (int round = 0; round < 4; ++round) {
                WriteJob w;
                ReadJob j;
                w.submit(m, f, 0, f.n, round % 2 == which);
                CHECK(j.submit(m, f, random_case(f, f.n, r), RKind::Rebuilt, round % 2 != which) == CEC_OK,
                      "job");
                CHECK(cec_multi_wait(m, j.id) == CEC_OK && cec_multi_wait(m, w.id) == CEC_OK, "wait");
                w.check(f);
                j.check(f);
            }
            cec_multi_free(m);
        };
        std::thread other(drive, 1);
        drive(0);
        other.join();
        finish();
    }
    // one thread allocates and frees cec_host_alloc buffers in a loop while a scheduler's workers
    // ask pinned_range about their jobs' buffers (a binding's buffer finaliser beside a job)
    {
        begin("d cec_host_alloc churn beside a scheduler seed=%llu", (unsigned long long)seed);
        set_schedule(seed, g_mutant);
        Codec codec(d, p);
        Rng r(seed);
        const Fix f = make_fix(d, p, L, 3 * P, seed);
        std::atomic<bool> stop{false};
        std::atomic<uint64_t> churned{0};
        std::thread churn([&] {
            Rng cr(seed + 99);
            std::vector<void*> live;
            while (!stop.load()) {
                void* q = nullptr;
                CHECK(cec_host_alloc(64 + cr.below(4096), cr.below(2) ? 0 : -1, &q) == CEC_OK, "churn alloc");
                CHECK(cec_host_is_pinned(q, 64) == 1, "a cec_host_alloc buffer is pinned");
                live.push_back(q);
                if (live.size() > 4) {
                    const size_t i = cr.below(live.size());
                    cec_host_free(live[i]);
                    live.erase(live.begin() + long(i));
                }
                churned.fetch_add(1);
            }
            for (void* q : live) cec_host_free(q);
        });
        {
            Multi mu(codec, L, P, depth, {0, 0});
            for (int round = 0; round < 12 || churned.load() < 50; ++round) {
                WriteJob w;
                ReadJob j;
                w.submit(mu.m, f, 0, f.n, round % 2 == 0);
                CHECK(j.submit(mu.m, f, random_case(f, f.n, r), RKind::Read, round % 3 == 0) == CEC_OK, "job");
                CHECK(cec_multi_wait(mu.m, w.id) == CEC_OK && cec_multi_wait(mu.m, j.id) == CEC_OK, "wait");
                w.check(f);
                j.check(f);
            }
            stop = true;
            churn.join();
        }
        finish();
    }
}

// ------------------------------------------------------------------------------------------
// e. Creation failures
// ------------------------------------------------------------------------------------------
void scenario_creation_failures() {
    const size_t d = 3, p = 2, L = 683, P = 4, depth = 2;
    struct Ctor {
        const char* name;
        int devices;
        std::function<int(const cec_codec*, std::string*)> make_and_free;
    };
    auto pipe = [&](const cec_codec* c, std::string* err) {
        cec_pipeline* pl = reinterpret_cast<cec_pipeline*>(uintptr_t(1));
        const int st = cec_pipeline_new_ex(c, L, P, depth, 0u, &pl);
        if (st != CEC_OK) *err = cec_pipeline_last_error();
        CHECK((st == CEC_OK) == (pl != nullptr), "status %d and pipeline %p disagree", st, (void*)pl);
        cec_pipeline_free(pl);
        return st;
    };
    auto rpipe = [&](unsigned flags) {
        return [=](const cec_codec* c, std::string* err) {
            cec_read_pipeline* pl = reinterpret_cast<cec_read_pipeline*>(uintptr_t(1));
            const int st = cec_read_pipeline_new_ex(c, L, P, depth, flags, &pl);
            if (st != CEC_OK) *err = cec_pipeline_last_error();
            CHECK((st == CEC_OK) == (pl != nullptr), "status %d and pipeline %p disagree", st, (void*)pl);
            cec_read_pipeline_free(pl);
            return st;
        };
    };
    auto multi = [&](std::vector<int> devices) {
        return [=](const cec_codec* c, std::string* err) {
            cec_multi* m = reinterpret_cast<cec_multi*>(uintptr_t(1));
            const int st = cec_multi_new_ex(c, L, P, depth, devices.data(), devices.size(),
                                            CEC_MULTI_WRITE | CEC_MULTI_READ, &m);
            if (st != CEC_OK) *err = cec_multi_last_error();
            CHECK((st == CEC_OK) == (m != nullptr), "status %d and scheduler %p disagree", st, (void*)m);
            cec_multi_free(m);
            return st;
        };
    };
    const Ctor ctors[] = {{"cec_pipeline_new_ex", 1, pipe},
                          {"cec_read_pipeline_new_ex", 1, rpipe(0u)},
                          {"cec_read_pipeline_new_ex CEC_READ_CARRY", 1, rpipe(CEC_READ_CARRY)},
                          {"cec_multi_new_ex on 1 shard", 1, multi({0})},
                          {"cec_multi_new_ex on [0,1]", 2, multi({0, 1})},
                          {"cec_multi_new_ex on [0,0]", 1, multi({0, 0})}};
    for (const Ctor& ct : ctors) {
        begin("e %s, clean", ct.name);
        standin_set_devices(ct.devices);
        Codec codec(d, p);
        std::string err;
        CHECK(ct.make_and_free(codec.c, &err) == CEC_OK, "the clean run fails: %s", err.c_str());
        uint64_t counts[5];
        size_t total = 0;
        for (int i = 0; i < 5; ++i) total += counts[i] = standin_calls(standin_creating_calls[i]);
        finish();
        size_t failed = 0;
        for (int i = 0; i < 5; ++i)
            for (uint64_t nth = 1; nth <= counts[i]; ++nth) {
                begin("e %s, %s call %llu of %llu fails", ct.name, standin_creating_calls[i],
                      (unsigned long long)nth, (unsigned long long)counts[i]);
                standin_set_devices(ct.devices);
                set_schedule(nth, g_mutant);
                standin_fail(standin_creating_calls[i], nth);
                err.clear();
                const int st = ct.make_and_free(codec.c, &err);
                CHECK(st == CEC_ERR_OUT_OF_MEMORY || st == CEC_ERR_HIP, "the constructor returns %d", st);
                CHECK(!err.empty(), "no message");
                finish();  // nothing live, no thread left, no violation
                ++failed;
            }
        CHECK(failed == total && total > 0, "no creating call");
        std::printf("e %s: %zu creating calls, each failed once\n", ct.name, total);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t first = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const uint64_t count = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 3;
    const char* only = std::getenv("SCHED_HOST_ONLY");
    auto want = [&](char c) { return !only || std::strchr(only, c); };
    if (const char* mt = std::getenv("SCHED_HOST_MUTANT")) {
        if (!std::strcmp(mt, "event_sync")) g_mutant = kMutantEventSyncNoWait;
        else if (!std::strcmp(mt, "stream_wait")) g_mutant = kMutantDropStreamWaitEvent;
        else {
            std::printf("unknown SCHED_HOST_MUTANT %s\n", mt);
            return 2;
        }
    }
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::thread([] {}).join();  // a sanitizer's own background thread starts with the first thread
    sleep_us(20000);
    g_base_threads = thread_count();
    if (want('s') && g_mutant == kMutantNone) standin_selftest();
    struct Shape {
        size_t d, p, L, P, depth;
    };
    // RS(3,2) and RS(10,4); L = 683 gives cs = 768 (the column-by-column copies); 4 to 6 parts
    // per batch; depth 1 to 3
    const Shape shapes[] = {{3, 2, 64, 4, 1}, {3, 2, 683, 5, 2}, {10, 4, 683, 4, 3},
                            {10, 4, 4096, 6, 2}, {3, 2, 4096, 4, 3}};
    const std::vector<std::vector<int>> layouts = {{0}, {0, 0}, {0, 1}};
    for (uint64_t seed = first; seed < first + count; ++seed) {
        size_t i = 0;
        for (const Shape& s : shapes) {
            if (want('a')) scenario_write(s.d, s.p, s.L, s.P, s.depth, seed);
            if (want('b')) scenario_read(s.d, s.p, s.L, s.P, s.depth, seed);
            if (want('b')) scenario_carry(s.d, s.p, s.L, s.P, s.depth, seed);
            if (want('c')) scenario_multi(s.d, s.p, s.L, s.P, s.depth, layouts[(i + seed) % 3], seed);
            ++i;
        }
        if (want('d')) scenario_lifecycle(seed);
    }
    if (want('e') && g_mutant == kMutantNone) scenario_creation_failures();
    standin_reset();
    std::printf("sched_host_test: %llu seeds, %llu checks, 0 failed\n", (unsigned long long)count,
                (unsigned long long)g_checks.load());
    return 0;
}
